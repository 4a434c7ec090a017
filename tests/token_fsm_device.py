"""The lockstep differential run behind tests/test_token_fsm_gpu.py (a plain helper module), on tests/sampler_adj_device.py's buffers.

Run A draws through gq_sample_topk_fsm / gq_sample_full_fsm with the machine's tables, masks built by gq_token_fsm_build and a device state
word; run B, draw for draw from the same state, through the existing entry (gq_sample_topk_lp / _lp_topn, gq_sample_full / _topn) with
`suppress` = token_fsm_model's mask row of the HOST-tracked state.  After every draw everything the draw writes is compared byte for byte,
A's state word against the model's transition, and the guards of A's buffers are checked.  A case with additive adjustments gives B the
host-adjusted logits (sampler_adj_model), so its raw log-probabilities and top-n rows are compared for the other cases only."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

import guarded
import sampler_adj_device as dev
import sampler_adj_model as am
import token_fsm_model as fm

EMPTY_TOKEN = fm.EMPTY_TOKEN
# base: a sampler_adj_model.Case (logits, filters, penalty, sets, ban, fold, adjustments); machine: (n_states, edges, default_next); start: the state
# the run begins in
FsmCase = namedtuple("FsmCase", "name base machine start")


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32).reshape(-1)


class FsmRun(dev.Run):
    """dev.Run with the machine next to it: fsm=True gives the run tables, masks and a state word and draws through the _fsm entry"""

    def __init__(self, fc, full, fsm=True, adjust=None, top_n=0, csr=None):
        from guidedquant_amd import _lib
        c = fc.base
        adjusted = bool(am.case_inputs(c)[1]) or c.fp != 0.0 or c.pp != 0.0 or bool(c.pre)
        super().__init__(c, full, adjusted if adjust is None else adjust, top_n)
        self.fc, self.fsm = fc, None
        if not fsm:
            return
        S, edges, dn = fc.machine
        self.csr = csr if csr is not None else fm.to_csr(S, edges, dn)
        W = fm.words(c.V)
        self.tables = [self.gi.inp(n, a if a.size else _i32([0])) for n, a in zip(("row_ptr", "edge_tok", "edge_next", "default_next"), self.csr)]
        self.masks = self.gi.out("masks", 4 * S * W)
        self.fsm_state = self.go.inp("fsm_state", _i32([fc.start]))
        _lib.check(self.L.gq_token_fsm_build(*(t.ptr() for t in self.tables), S, c.V, guarded.ptr(self.sup), self.masks.ptr(), self.stream), "gq_token_fsm_build")
        self.fsm = _lib.GqTokenFsm(self.masks.ptr(), W, S, *(t.ptr() for t in self.tables), self.fsm_state.ptr())
        torch.cuda.synchronize()

    def state_word(self):
        return int(self.fsm_state.view(torch.int32)[0])

    def draw(self, i, expect=0, **over):
        name = over.get("entry", ("gq_sample_full_fsm" if self.full else "gq_sample_topk_fsm") if self.fsm is not None else None)
        if name is None or not name.endswith("_fsm"):
            return super().draw(i, expect, **over)
        # (Run.draw's arguments of the _adj entry, then the machine in front of the stream)
        c, p = self.c, guarded.ptr
        head = (self.logits.ptr(), over.get("V", c.V), over.get("top_k", c.top_k), c.top_p)
        tail = (self.tok.ptr(), self.pos.ptr(), self.nt.ptr() + 4 * i, p(self.ban), self.seq.ptr(), self.seq_cap, p(self.table),
                self.xo.ptr() + 2 * c.dim * i if c.dim else None, c.dim, self.ssq.ptr() + 4096 * i if c.dim else None, c.rp, p(self.seen), p(self.sup))
        lps = (self.lraw.ptr(), self.ldrawn.ptr(), dev.lp_cap(c))
        topn = (over.get("top_n", self.top_n), p(self.top_ids), p(self.top_lps), p(self.topn_ws))
        adj, fsm = over.get("adj", self.adj), over.get("fsm", self.fsm)
        if self.full:
            a = head + (c.min_p, c.T, c.seed, self.ctr.ptr(), self.ws.ptr(), self.ws_bytes) + tail + lps
        else:
            a = head + (c.T, c.seed, self.ctr.ptr(), self.wv.ptr(), self.wi.ptr()) + tail + (self.lws.ptr(), ) + lps
        a += topn + (ctypes.byref(adj) if adj is not None else None, ctypes.byref(fsm) if fsm is not None else None)
        rc = getattr(self.L, name)(*a, self.stream)
        assert rc == expect, (c.name, name, i, rc, self.L.gq_last_error())


DRAW_STATE = dev.DRAW_STATE
RAW_STATE = ("lraw", "top_ids", "top_lps")  # (compared where B draws from the raw logits)


def lockstep(fc, full, top_n=0):
    """A and B in lockstep with every per-draw check; returns (the tokens, the states the machine went through)"""
    c = fc.base
    A = FsmRun(fc, full, True, None, top_n)
    B = FsmRun(fc, full, False, False, top_n)
    V, W = c.V, fm.words(c.V)
    base = A.sup.numpy(np.uint32) if A.sup is not None else None
    rows = fm.mask_rows(*A.csr, V, base)
    assert np.array_equal(A.masks.numpy(np.uint32).reshape(-1, W), rows), (fc.name, "the mask rows")
    if B.sup is None:
        B.sup = B.gi.out("suppress", 4 * W)
    rows_dev = torch.from_numpy(rows.view(np.int32)).cuda()
    adjusted = A.adjust
    counts = A.pre.copy()
    entry_b = ("gq_sample_full_topn" if full else "gq_sample_topk_lp_topn") if top_n else ("gq_sample_full" if full else "gq_sample_topk_lp")
    s, tokens, states = fc.start, [], [fc.start]
    for i in range(c.n):
        A.draw(i)
        A.go.check()  # (synchronises)
        B.sup.view(torch.int32).copy_(rows_dev[s])
        if adjusted:
            B.set_logits(am.adjusted_logits(A.raw, A.bias, counts, c.fp, c.pp))
        B.draw(i, entry=entry_b)
        torch.cuda.synchronize()
        ta, tb = int(A.nt.view(torch.int32)[i]), int(B.nt.view(torch.int32)[i])
        assert ta == tb, (fc.name, "draw", i, "state", s, ta, tb)
        for k in ("tok", "pos", "ctr"):
            va, vb = int(getattr(A, k).view(torch.int32)[0]), int(getattr(B, k).view(torch.int32)[0])
            assert va == vb, (fc.name, "draw", i, k, va, vb)
        assert int(A.tok.view(torch.int32)[0]) == ta and int(A.pos.view(torch.int32)[0]) == c.pos0 + i + 1 and int(A.ctr.view(torch.int32)[0]) == i + 1
        for k in DRAW_STATE + (() if adjusted else RAW_STATE):
            a, b = getattr(A, k), getattr(B, k)
            if a is not None:
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (fc.name, "draw", i, k)
        if full:  # the workspace report {n, n_k, Z_k, Z_kept}
            assert torch.equal(A.ws.view(torch.uint8)[:24], B.ws.view(torch.uint8)[:24]), (fc.name, "draw", i, "report")
        if 0 <= ta < V:
            assert (rows[s, ta >> 5] >> np.uint32(ta & 31)) & 1 == 0, (fc.name, "draw", i, "a forbidden token was drawn", s, ta)
            counts[ta] += 1
        else:
            assert ta == EMPTY_TOKEN
        s = fm.step(*A.csr, V, s, ta)
        got = A.state_word()
        assert got == s, (fc.name, "draw", i, "state", got, s, ta)
        tokens.append(ta)
        states.append(s)
    for r in (A, B):
        r.go.check()
        r.gi.check()
    assert np.array_equal(A.masks.numpy(np.uint32).reshape(-1, W), rows), (fc.name, "a draw wrote the masks")
    for t, a in zip(A.tables, A.csr):
        assert np.array_equal(t.numpy(np.int32)[:a.size], a), (fc.name, "a draw wrote the tables")
    return tokens, states
