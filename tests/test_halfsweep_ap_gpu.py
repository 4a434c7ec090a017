"""GPU: every finite fp16 gate through the SiLU * up sites of the decode path -- the pair epilogue (GQ_EPI_SILU_PAIRS) and the SiLU prologue
(GQ_PRO_SILU_MUL) of gq_anyprec_gemv_fused -- family by family, against the candidate sets of tests/halfsweep_model.py at
DELTA_DECODE = 2^-16 (test_ap_exact_fused_gpu.DELTA: the __expf sites).

The families and their knobs are those of tests/test_bounds_ap_gemv_gpu.py (ENV / set_env); every launch asserts its route.  A family
runs at the smallest K, and the lowest bit width, of its CASES rows that list the form.  The GEMV around the site is made a selector
(halfsweep_model.pair_selector / prologue_selector), so that the site's input and output are visible element by element:

pair epilogue   x is one-hot, every row has code 0 in column 0 and code 1 elsewhere, lut[r] = [v_r, 0, ...]: y[r] = v_r.  Even rows plant
                the finite gate patterns, odd rows scramble_finite of them (another finite pattern for every gate).  The unpaired launch
                on the same route must return the planted values (-0 as +0): the case reaches the whole domain.  The paired launch's
                out[i] must then be one of pair_candidates(y[2i], y[2i + 1], DELTA_DECODE), NaN by class and zeros with their sign.
                N = 16 384 rows per launch (4096 for plane-local: the local image serves no more), 8 (32) launches.
SiLU prologue   N = K, row r has code 0 in column r only, lut[r] = [1, 0, ...]: y = the activation vector the prologue formed.  x = [g | u]
                with u = 2^-e (halfsweep_model.prologue_ups), so that every product and every partial sum any kernel forms is exact in
                fp32, the bit-plane sums of the plane and stream kernels included.  y[r] must be u_r times a SiLU candidate of g_r; where
                the candidate is zero, values are compared, not signs.  The plain launch on the primary products h must return h bit
                for bit (-0 as +0) -- it does for every family here; a family for which it did not would be listed in INEXACT_PLAIN and
                checked against its own plain launch at the gates with one candidate.
Only finite gates can be planted: a NaN or an Inf in a GEMV's lut or activations reaches every row.  The non-finite gates are swept at
the expf site (tests/test_halfsweep_rows_gpu.py), which shares the expression.

QTIP is out of scope: its three SiLU * up sites (csrc/qtip.hip) feed a Hadamard transform before anything observable, so no element-wise
view of them exists.

Measured on an MI355X (outputs that are not the primary candidate; the non-primary gate of largest |g|) -- no value outside its candidates:
  pair epilogue   4 of 65 536 pairs, largest |g| -2.7246, in each of dq, exact, pair-table, plane, plane-local, stream, wide
  SiLU prologue   3 of 63 488 gates, largest |g| -2.7246, in each of the same seven families
(the seven share one expression, g / (1 + __expf(-g)); the few gates it rounds the other way lie within 2^-24 of a tie.)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import halfsweep_model as hs  # noqa: E402
import test_bounds_ap_gemv_gpu as t  # noqa: E402
from ap_helpers import assert_route  # noqa: E402
from test_bounds_ap_gemv_gpu import _restore_env  # noqa: E402,F401  (autouse: the GQ_* environment and the mode are put back)

GQ_PRO_SILU_MUL, GQ_EPI_SILU_PAIRS = 2, 4
PAIR_ROWS = 16384
INEXACT_PLAIN = ()   # families whose plain launch does not return the prologue's products bit for bit: none


def families(form):
    """family -> (bits, K): the lowest bit width and the smallest K among the CASES rows whose forms list `form`"""
    out = {}
    for fam, bits, _, K, forms, _ in t.CASES:
        if form in forms:
            b0, k0 = out.get(fam, (bits, K))
            out[fam] = (min(b0, bits), min(k0, K))
    return out


PAIR_FAMILIES, SILU_FAMILIES = families("pairs"), families("silu")


class Layer:
    """one selector layer on the device; run() launches gq_anyprec_gemv_fused on it with the lut and activations of a step of the sweep"""

    def __init__(self, q, bits, fam):
        self.d = torch.device("cuda:0")
        self.q, self.bits, self.fam = torch.from_numpy(np.ascontiguousarray(q)).to(self.d), bits, fam
        self.N, self.K = q.shape[1], q.shape[2] * 32

    def run(self, x, lut, flags=0, out_elems=None):
        from guidedquant_amd import _lib
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float16)).to(self.d)
        lt = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float16)).to(self.d)
        out = torch.full((out_elems or self.N, ), float("nan"), dtype=torch.float16, device=self.d)
        rc = _lib.lib().gq_anyprec_gemv_fused(xt.data_ptr(), out.data_ptr(), self.q.data_ptr(), lt.data_ptr(), self.N, self.K, self.bits, None, 1e-5, None,
                                              flags, _lib.current_stream_ptr())
        _lib.check(rc, "gq_anyprec_gemv_fused")
        assert_route(self.fam)
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _pair_rows(fam, K, bits):
    """the largest N <= PAIR_ROWS (halving) at which the family serves both launches"""
    from guidedquant_amd import _lib
    N = PAIR_ROWS
    while N >= 256 and not all(_lib.ap_plan_route(N, K, bits, 1, False, f, 0)[0] == fam for f in (0, GQ_EPI_SILU_PAIRS)):
        N //= 2
    assert N >= 256, f"{fam} serves no selector of {K} columns"
    return N


def _worst(gates):
    return "none" if not gates.size else repr(float(gates[np.argmax(np.abs(gates))]))


@pytest.mark.parametrize("fam", sorted(PAIR_FAMILIES))
def test_pair_epilogue_over_every_finite_gate(fam):
    bits, K = PAIR_FAMILIES[fam]
    t.set_env(fam)
    N = _pair_rows(fam, K, bits)
    P = N // 2
    gate = np.concatenate([hs.FINITE, hs.FINITE[:65536 - hs.FINITE.size]])   # (65 536 pairs: whole launches)
    up = hs.scramble_finite(gate, 0)
    q, lut, x = hs.pair_selector(np.zeros(N, dtype=np.float16), K, bits)
    layer = Layer(q, bits, fam)
    nonprimary, seen, worst = 0, [], []
    for lo in range(0, gate.size, P):
        v = np.stack([gate[lo:lo + P], up[lo:lo + P]], axis=1).reshape(-1)
        lut[:, 0] = hs.half(v)
        y = layer.run(x, lut)
        arrived = hs.same(y, hs.half(v), zero_signs=False)
        assert arrived.all(), "%s: %d planted values did not arrive, first (planted, got) bits %s" % (
            fam, int((~arrived).sum()), [(hex(v[i]), hex(hs.bits(y)[i])) for i in np.flatnonzero(~arrived)[:4]])
        assert (hs.bits(y)[hs.half(v) == 0] == 0).all()   # -0 arrives as +0
        out = layer.run(x, lut, flags=GQ_EPI_SILU_PAIRS, out_elems=P)
        g, u = y[0::2], y[1::2]
        ok, npri = hs.in_candidates(out, hs.pair_candidates(g, u, hs.DELTA_DECODE))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, "%s: %d pair outputs outside their candidates; (gate, up, got) bits: %s" % (
            fam, bad.size, [(hex(hs.bits(g)[i]), hex(hs.bits(u)[i]), hex(hs.bits(out)[i])) for i in bad[:6]])
        nonprimary += int(npri.sum())
        worst.append(g[npri])
        seen.append(hs.bits(g))
    assert np.setdiff1d(hs.FINITE, np.concatenate(seen)).tolist() == [0x8000]   # every finite gate but -0 went through the site
    worst = np.concatenate(worst)
    print(f"pairs {fam} (bits {bits}, K {K}, N {N}): {nonprimary} of {gate.size} non-primary, largest |g| among them {_worst(worst)}")


@pytest.mark.parametrize("fam", sorted(SILU_FAMILIES))
def test_silu_prologue_over_every_finite_gate(fam):
    from guidedquant_amd import _lib
    bits, K = SILU_FAMILIES[fam]
    t.set_env(fam)
    for flags in (0, GQ_PRO_SILU_MUL):
        assert _lib.ap_plan_route(K, K, bits, 1, False, flags, 0)[0] == fam
    q, lut = hs.prologue_selector(K, bits)
    layer = Layer(q, bits, fam)
    n = -(-hs.FINITE.size // K) * K
    gate = hs.half(np.concatenate([hs.FINITE, hs.FINITE[:n - hs.FINITE.size]]))
    up = hs.prologue_ups(gate)
    cand = hs.pair_candidates(gate, up, hs.DELTA_DECODE)
    one = hs.same(cand[0], cand[2])
    nonprimary = np.zeros(n, dtype=bool)
    for lo in range(0, n, K):
        s = slice(lo, lo + K)
        h = cand[1][s]
        plain = layer.run(h, lut)
        exact = hs.same(plain, h, zero_signs=False)
        assert bool(exact.all()) == (fam not in INEXACT_PLAIN), f"{fam}: the plain launch returns the products exactly: {bool(exact.all())}"
        y = layer.run(np.concatenate([gate[s], up[s]]), lut, flags=GQ_PRO_SILU_MUL)
        if fam in INEXACT_PLAIN:
            ok, npri = hs.same(y, plain, zero_signs=False) | ~one[s], np.zeros(K, dtype=bool)
        else:
            ok, npri = hs.in_candidates(y, cand[:, s], zero_signs=False)
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, "%s: %d prologue outputs outside their candidates; (gate, up, got, primary) bits: %s" % (
            fam, bad.size, [(hex(hs.bits(gate[s])[i]), hex(hs.bits(up[s])[i]), hex(hs.bits(y)[i]), hex(hs.bits(h)[i])) for i in bad[:6]])
        nonprimary[s] = npri
    nonprimary[hs.FINITE.size:] = False   # (the padding repeats gates)
    print(f"prologue {fam} (bits {bits}, K {K}): {int(nonprimary.sum())} of {hs.FINITE.size} non-primary, largest |g| among them {_worst(gate[nonprimary])}")
