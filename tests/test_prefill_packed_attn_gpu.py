"""GPU: the packed prompt attention (csrc/prefill_attn.hip, gq_attn_prefill_packed) through the C ABI on guard-banded, poisoned buffers
(tests/guarded.py), against the one-sequence entry gq_attn_prefill and the host model tests/prefill_packed_model.py.

Cases: S in {1, 63, 64, 65, 131} x the segment layouts of prefill_packed_model.layouts (one segment; every segment one row; boundaries at
the rows 1, 63, 64, 65; a segment astride an edge of the query-tile and of the key-tile grid), with head_dim {64, 128}, head groups
{1, 4}, windows {0, 2, 65} and the data {random normal, hi300, cur_above} rotating along them (every value of every axis is met: asserted).
Cache rows >= S hold NaN / +-Inf / 65504 (prefill_attn_model.poison_rows).

  1. one segment: `out` is gq_attn_prefill(start = 0)'s with the same window, bit for bit -- every S x window.
  2. every row i is row i of gq_attn_prefill(S = i + 1, start = 0, window = w_i), w_i = min(i - seg_begin[i] + 1, window or inf), bit for
     bit: one small launch per row, on one case per S (324 launches).
  3. against the float64 reference within prefill_attn_model.error_bound(S, max|V|) (the derived bound of the one-sequence kernel).
  4. guard bands and every cache byte untouched.
  5. isolation: the K / V rows of every second segment overwritten with NaN / +-Inf / 65504 rows -- the rows of the other segments are
     bit-identical and finite (the odd segments, then the even ones).
  6. the argument checks return their codes and write nothing."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes  # noqa: E402
import prefill_attn_model as pam  # noqa: E402
import prefill_packed_model as ppm  # noqa: E402
from guarded import Guards  # noqa: E402

BQ, BK = 64, 64
SS = (1, 63, 64, 65, 131)
HDS, GROUPS, WINDOWS, DATA = (64, 128), (1, 4), (0, 2, 65), ("random", "hi300", "cur_above")


def _L():
    from guidedquant_amd import _lib
    return _lib


def _cases():
    """(S, layout, head_dim, group, window, data): every S x layout pair; the other axes rotate with co-prime periods"""
    cases, n = [], 0
    for S in SS:
        for name in ppm.layouts(S, BQ, BK):
            cases.append((S, name, HDS[n % 2], GROUPS[(n // 2) % 2], WINDOWS[n % 3], DATA[(n + n // 3) % 3]))
            n += 1
    for axis, vals in ((2, HDS), (3, GROUPS), (4, WINDOWS), (5, DATA)):
        assert {c[axis] for c in cases} == set(vals), (axis, {c[axis] for c in cases})
    multi = [c for c in cases if c[1] != "one"]  # (the segment boundaries meet every window, head_dim and kind of data too)
    for axis, vals in ((2, HDS), (4, WINDOWS), (5, DATA)):
        assert {c[axis] for c in multi} == set(vals), (axis, {c[axis] for c in multi})
    return cases


CASES = _cases()
_IDS = ["S%d-%s-hd%d-G%d-W%d-%s" % c for c in CASES]
# check 2, one case per S: the layout with the most boundaries that S has
PER_ROW = [next(c for c in CASES if c[0] == S and c[1] == name) for S, name in ((1, "one"), (63, "cuts"), (64, "ones"), (65, "astride"), (131, "cuts"))]


def _inputs(S, hd, G, data):
    H, Hkv = (2, 2) if G == 1 else (4, 1)
    scale = attn_probes.default_scale(hd)
    q, K, V = pam.profile_probe(data, H, Hkv, hd, S, 0, S + 3, scale, BK)  # (rows >= S poisoned)
    return H, Hkv, scale, q, K, V


def _packed(q, K, V, sb, S, H, Hkv, hd, scale, window, max_seq=None):
    """the guarded launch: (rc, out, the guards)"""
    L = _L()
    g = Guards()
    bq, bk, bv, bs = g.inp("q", q), g.inp("k_cache", K), g.inp("v_cache", V), g.inp("seg_begin", sb)
    bo = g.out("out", max(S, 1) * H * hd * 2)
    rc = L.lib().gq_attn_prefill_packed(bq.ptr(), bk.ptr(), bv.ptr(), None if sb is None else bs.ptr(), bo.ptr(), S, H, Hkv, hd,
                                        K.shape[1] if max_seq is None else max_seq, scale, window, None)
    g.check()
    # (check 4: the kernel reads the caches, never writes them)
    assert torch.equal(bk.view(torch.int16).cpu(), K.reshape(-1).view(torch.int16)) and torch.equal(bv.view(torch.int16).cpu(), V.reshape(-1).view(torch.int16))
    return rc, bo.view(torch.int16, (max(S, 1), H * hd)).cpu()


def _one_sequence(qd, Kd, Vd, S, H, Hkv, hd, scale, window):
    """gq_attn_prefill(S, start = 0) on device tensors: out int16 bits [S, H * hd]"""
    L = _L()
    qs = qd[:, :S].contiguous()
    out = torch.empty(S, H * hd, dtype=torch.float16, device=qd.device)
    L.check(L.lib().gq_attn_prefill(qs.data_ptr(), Kd.data_ptr(), Vd.data_ptr(), out.data_ptr(), S, 0, H, Hkv, hd, Kd.shape[1], scale, window, None), "gq_attn_prefill")
    torch.cuda.synchronize()
    return out.view(torch.int16).cpu()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("S", SS)
def test_one_segment_is_the_one_sequence_launch_bit_for_bit(S, window):
    d = torch.device("cuda:0")
    n = SS.index(S) + WINDOWS.index(window)
    hd, G, data = HDS[n % 2], GROUPS[(n // 2) % 2], DATA[n % 3]
    H, Hkv, scale, q, K, V = _inputs(S, hd, G, data)
    rc, got = _packed(q, K, V, torch.zeros(S, dtype=torch.int32), S, H, Hkv, hd, scale, window)
    assert rc == 0, _L().lib().gq_last_error()
    want = _one_sequence(q.to(d), K.to(d), V.to(d), S, H, Hkv, hd, scale, window)
    assert torch.equal(got, want), "%d element(s) differ" % int((got != want).sum())


@pytest.mark.parametrize("S,layout,hd,G,window,data", CASES, ids=_IDS)
def test_against_float64_and_isolation(S, layout, hd, G, window, data):
    lens = ppm.layouts(S, BQ, BK)[layout]
    sb = ppm.seg_begin_of(lens)
    H, Hkv, scale, q, K, V = _inputs(S, hd, G, data)
    rc, bits = _packed(q, K, V, sb, S, H, Hkv, hd, scale, window)
    assert rc == 0, _L().lib().gq_last_error()
    got = bits.view(torch.float16).double()
    assert bool(torch.isfinite(got).all())
    want = ppm.reference(q, K, V, sb, scale, window)
    vmax = float(V[:, :S].float().abs().max())
    err, bound = float((got - want).abs().max()), pam.error_bound(S, vmax)
    print("S%d %s hd%d G%d W%d %s: max|V| %.3f  kernel %.3e  bound %.3e" % (S, layout, hd, G, window, data, vmax, err, bound))
    assert err <= bound, (err, bound)
    if len(lens) == 1:
        return
    # isolation: every second segment's cache rows poisoned (whole rows of NaN, +Inf, -Inf, 65504 in a cycle), the others must not move
    seg_of_row = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    poison = torch.tensor(pam.POISON_BITS, dtype=torch.int32).to(torch.int16).view(torch.float16)
    for parity in (1, 0):
        hit = (seg_of_row % 2) == parity
        K2, V2 = K.clone(), V.clone()
        rows = torch.nonzero(hit).reshape(-1)
        K2[:, rows] = poison[rows % 4][None, :, None]
        V2[:, rows] = poison[rows % 4][None, :, None]
        rc, bits2 = _packed(q, K2, V2, sb, S, H, Hkv, hd, scale, window)
        assert rc == 0
        keep = ~hit
        assert bool(torch.isfinite(bits2.view(torch.float16)[keep].float()).all()), "a poisoned segment reached another segment's rows"
        assert torch.equal(bits2[keep], bits[keep]), "%d element(s) of untouched segments moved" % int((bits2[keep] != bits[keep]).sum())


@pytest.mark.parametrize("S,layout,hd,G,window,data", PER_ROW, ids=["S%d-%s-hd%d-G%d-W%d-%s" % c for c in PER_ROW])
def test_every_row_is_a_one_sequence_launch_bit_for_bit(S, layout, hd, G, window, data):
    d = torch.device("cuda:0")
    sb = ppm.seg_begin_of(ppm.layouts(S, BQ, BK)[layout])
    H, Hkv, scale, q, K, V = _inputs(S, hd, G, data)
    rc, got = _packed(q, K, V, sb, S, H, Hkv, hd, scale, window)
    assert rc == 0, _L().lib().gq_last_error()
    qd, Kd, Vd = q.to(d), K.to(d), V.to(d)
    bad = []
    for i, w in enumerate(ppm.row_window(sb, window)):
        want = _one_sequence(qd, Kd, Vd, i + 1, H, Hkv, hd, scale, w)[i]
        if not torch.equal(got[i], want):
            bad.append((i, w, int((got[i] != want).sum())))
    assert not bad, "rows (row, window, elements) that differ from their one-sequence launch: %r" % bad[:8]


def test_argument_checks_write_nothing():
    L = _L()
    S, hd = 5, 64
    H, Hkv, scale, q, K, V = _inputs(S, hd, 1, "random")
    sb = torch.zeros(S, dtype=torch.int32)
    untouched = lambda bits: bool((bits == 0x7E7E).all())  # noqa: E731  (the poison pattern)
    for args, want in (((q, K, V, sb, 0, H, Hkv, hd, scale, 0), L.GQ_EINVAL),        # no rows
                       ((q, K, V, None, S, H, Hkv, hd, scale, 0), L.GQ_EINVAL),      # a null seg_begin
                       ((q, K, V, sb, S, H, Hkv, hd, scale, 0, S - 1), L.GQ_EINVAL),  # S > max_seq
                       ((q, K, V, sb, S, 3, 2, hd, scale, 0), L.GQ_ENOTSUP),         # n_head no multiple of n_kv_head
                       ((q[:, :, :32].contiguous(), K[:, :, :32].contiguous(), V[:, :, :32].contiguous(), sb, S, H, Hkv, 32, scale, 0), L.GQ_ENOTSUP)):
        rc, bits = _packed(*args)
        assert rc == want, (rc, want)
        assert untouched(bits)
    # a malformed array (entries beyond their row, negative ones): numbers may be wrong, every access stays inside rows [0, S)
    rc, bits = _packed(q, K, V, torch.tensor([3, -1, 100, 0, 0x7FFFFFFF], dtype=torch.int32), S, H, Hkv, hd, scale, 0)
    assert rc == 0 and bool(torch.isfinite(bits.view(torch.float16).float()).all())
