"""GPU: gq_token_fsm_build, gq_sample_topk_fsm and gq_sample_full_fsm through the C ABI, on guarded and poisoned buffers.

The builder: its mask rows against tests/token_fsm_model.py at every vocabulary, with 1, 3 and 40 states, rows of 0, 1, 2 and 33 edges, edges
at tokens 0, 31, 32 and V - 1, default-allowed states with forbidden exceptions, with and without a base set, the tail bits of the last word.

The draws (tests/token_fsm_device.py has the run), in lockstep over 64 to 128 draws per case: A = the _fsm entry, B = for each draw the
existing entry from the same state with `suppress` = the model's mask row of the host-tracked state.  After every draw next_tok, tok_io,
pos_io, counter, seq_out, seen, x_out, ssq_out, lp_drawn, lp_raw and the top-n rows are equal byte for byte, state[0] equals the model's, no
forbidden token was drawn and the guards hold."""
import numpy as np
import pytest

import guarded
import sampler_adj_model as am
import token_fsm_device as dev
import token_fsm_model as fm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("V", [1, 33, 300, 4096, 131073, 262144])
def test_the_mask_builder(V):
    from guidedquant_amd import _lib
    L, s = _lib.lib(), _lib.current_stream_ptr()
    W = fm.words(V)
    for S in (1, 3, 40):
        Sn, edges, dn = fm.builder_machine(S, V, seed=V % 97)
        csr = fm.to_csr(Sn, edges, dn)
        lens = set(np.diff(csr[0]).tolist())
        assert lens == {min(n, V) for n in (0, 1, 2, 33)[:min(S, 4)]}, "rows of 0, 1, 2 and 33 edges"
        if S == 40:
            assert set(fm.layout_edges(V)) <= set(csr[1].tolist()), "edges at tokens 0, 31, 32 and V - 1"
        base_ids = sorted({0, V - 1, V // 2, min(33, V - 1)})
        base = np.zeros(W, dtype=np.uint32)
        for t in base_ids:
            base[t >> 5] |= np.uint32(1 << (t & 31))
        for with_base in (False, True):
            g = guarded.Guards()
            tabs = [g.inp(n, a if a.size else np.zeros(1, dtype=np.int32)) for n, a in zip(("row_ptr", "edge_tok", "edge_next", "default_next"), csr)]
            gb = g.inp("base", base) if with_base else None
            masks = g.out("masks", 4 * S * W)
            assert L.gq_token_fsm_build(*(t.ptr() for t in tabs), S, V, guarded.ptr(gb), masks.ptr(), s) == 0
            g.check()
            got = masks.numpy(np.uint32).reshape(S, W)
            want = fm.mask_rows(*csr, V, base if with_base else None)
            assert np.array_equal(got, want), (V, S, with_base, np.nonzero((got != want).any(axis=1))[0][:4])
            if V % 32:  # the bits at and past V in the last word are set, whatever the row
                assert ((got[:, -1] >> np.uint32(V % 32)) == np.uint32(0xFFFFFFFF) >> np.uint32(V % 32)).all()
            # what a row says: a default-forbidding state allows exactly its allowing edges, minus the base set
            for st in range(S):
                if dn[st] < 0 and V <= 4096:
                    allow = sorted(t for (q, t, n) in edges if q == st and n >= 0 and not (with_base and t in base_ids))
                    assert fm.row_allowed(got[st], V).tolist() == allow


# ------------------------------------------------------------------------------------------------ the cases of the differential
def _hot(c, n=12):
    """the n tokens the case's logits favour"""
    x = am.case_logits(c).astype(np.float32)
    return np.argsort(-np.nan_to_num(x, nan=-np.inf), kind="stable")[:n].tolist()


def _ring(name, full, V, top_k, start=0, S=5, **kw):
    c = am._case(name, V, kw.pop("prof", "gauss"), top_k, kw.pop("T", 1.0), **kw)
    return dev.FsmCase(name, c, fm.ring_machine(V, S, seed=len(name), hot=_hot(c)), start), full


_NAN = float("nan")
CASES = dict([
    # both samplers at the three vocabularies (the narrow and the wide instances), top_k 1 / 50 / 64 and 0 / 200
    *[(n, _ring(n, False, V, k, n=128 if V <= 4096 else 64, seed=i, T=0.0 if k == 1 else 1.0)) for i, (V, k) in enumerate(((33, 1), (4096, 50), (151936, 64), (33, 50), (4096, 1)))
      for n in ("topk_v%d_k%d" % (V, k), )],
    *[(n, _ring(n, True, V, k, n=128 if V <= 4096 else 64, seed=i)) for i, (V, k) in enumerate(((33, 0), (4096, 200), (151936, 0), (151936, 200)))
      for n in ("full_v%d_k%d" % (V, k), )],
    # the filters
    ("topk_top_p", _ring("topk_top_p", False, 4096, 50, prof="quant", top_p=0.9, n=128)),
    ("full_top_p_min_p", _ring("full_top_p_min_p", True, 4096, 0, prof="quant", top_p=0.9, min_p=0.05, n=128)),
    # a repetition penalty with the additive adjustments on top, a suppress list (the builder's base) and log-probability slots that end early
    ("topk_rp_adjust", _ring("topk_rp_adjust", False, 4096, 8, fp=0.4, pp=0.2, bias="layout", pre="layout", rp=1.3, seen0=(0, 31, 32, 100, 101), suppress=(1, 2, 4095), n=128)),
    ("full_rp_adjust", _ring("full_rp_adjust", True, 4096, 200, fp=0.4, pp=0.2, bias="layout", pre="layout", rp=1.3, seen0=(0, 31, 32, 100, 101), suppress=(1, 2, 4095), top_p=0.9,
                             n=128)),
    ("topk_rp_suppress", _ring("topk_rp_suppress", False, 4096, 50, rp=1.3, seen0=(0, 31, 32, 100, 101), suppress=(1, 2, 4095), n=128, lp_cut=20)),
    # an expiring ban, from a position other than 0
    ("topk_ban", _ring("topk_ban", False, 4096, 50, ban=(2, 40, (0, 31)), pos0=17, n=128)),
    ("full_ban", _ring("full_ban", True, 4096, 0, ban=(2, 40, (0, 31)), pos0=17, n=128)),
    # the embedding fold, two widths
    ("topk_embed_fold", _ring("topk_embed_fold", False, 4096, 50, dim=64, n=64)),
    ("full_embed_fold_wide", _ring("full_embed_fold_wide", True, 151936, 0, dim=8, min_p=0.05, n=64)),
    # a start state other than 0 with many states: a wrong stride or a wrong row shows in the first draw
    ("topk_start_state", _ring("topk_start_state", False, 300, 50, start=37, S=40, n=128)),
    ("full_start_state", _ring("full_start_state", True, 300, 0, start=37, S=40, n=128)),
])
# a chain: every state allows exactly one token, so the drawn sequence is the chain whatever the logits say
_CHAIN = [0, 31, 32, 4095, 7, 7, 100, 2047, 2048, 64, 63]
for _full in (False, True):
    _n = ("full" if _full else "topk") + "_chain"
    CASES[_n] = (dev.FsmCase(_n, am._case(_n, 4096, "gauss", 0 if _full else 50, 1.0, n=64), fm.chain_machine(_CHAIN), 3), _full)
    # state 1 allows only tokens whose logits are NaN: the token of an empty candidate set, and the state stays
    _n = ("full" if _full else "topk") + "_nan_state"
    CASES[_n] = (dev.FsmCase(_n, am._case(_n, 300, "gauss", 0 if _full else 50, 1.0, plant=((5, _NAN), (299, _NAN)), n=64), (2, [(0, 9, 1), (1, 5, 0), (1, 299, 0)], [-1, -1]), 0),
                 _full)
TOP_N = {"topk_v4096_k50": 3, "full_v4096_k200": 5, "topk_rp_suppress": 20, "full_ban": 2, "topk_start_state": 1}
_TOKENS = {}


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    assert torch.cuda.is_available()
    fc, full = CASES[name]
    tokens, states = dev.lockstep(fc, full, TOP_N.get(name, 0))
    _TOKENS[name] = tokens
    if name.endswith("_chain"):
        assert tokens == [_CHAIN[(3 + i) % len(_CHAIN)] for i in range(fc.base.n)]
    elif name.endswith("_nan_state"):
        assert tokens == [9] + [dev.EMPTY_TOKEN] * (fc.base.n - 1) and states == [0] + [1] * fc.base.n
    else:
        if fc.base.top_k != 1:
            assert len(set(states)) >= 2 and len(set(tokens)) > 4, "the run went through the machine"


@pytest.mark.parametrize("full", [False, True])
def test_the_mask_changes_the_draw(full):
    """the differential has something to show: the same seeds without the machine draw other tokens"""
    name = "full_v4096_k200" if full else "topk_v4096_k50"
    fc, _ = CASES[name]
    constrained = _TOKENS.get(name) or dev.lockstep(fc, full, TOP_N[name])[0]
    plain = dev.FsmRun(fc, full, False, False)
    for i in range(fc.base.n):
        plain.draw(i)
    torch.cuda.synchronize()
    assert plain.nt.numpy(np.int32)[:fc.base.n].tolist() != constrained


@pytest.mark.parametrize("full", [False, True])
def test_no_machine_and_a_free_machine_draw_what_the_adj_entry_draws(full):
    """fsm == NULL is the _adj entry's call; a machine with one state that allows everything forbids nothing: both bit for bit"""
    fc, _ = CASES["full_rp_adjust" if full else "topk_rp_adjust"]
    free = fc._replace(machine=(1, [], [0]), start=0)
    entry = "gq_sample_full_fsm" if full else "gq_sample_topk_fsm"
    old = dev.FsmRun(fc, full, False, None, 4)
    for i in range(fc.base.n):
        old.draw(i, entry="gq_sample_full_adj" if full else "gq_sample_topk_adj")
    old.go.check()
    want = old.state()
    for run in (dev.FsmRun(fc, full, False, None, 4), dev.FsmRun(free, full, True, None, 4)):
        for i in range(fc.base.n):
            run.draw(i, entry=entry)
        run.go.check()
        run.gi.check()
        got = run.state()
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(want[k], got[k]), (k, run.fsm is None)
        if run.fsm is not None:
            assert run.state_word() == 0
