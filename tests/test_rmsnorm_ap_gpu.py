"""GPU: every finite fp16 value through the RMSNorm prologues of the decode step's GEMV launches -- gq_anyprec_gemv_fused with a norm
weight, family by family (exact, pair-table, wide, plane, stream, dq: the knobs of tests/test_bounds_ap_gemv_gpu.py, every launch
asserts its route), the stream kernel's hand-over form (gq_anyprec_gemv_fused_ho with ssq_in from gq_ssq_rows), the fused q/k/v launch
(gq_anyprec_gemv_qkv_rope) and the lm_head prologue (gq_dense_gemv_f16) -- against the candidate sets of tests/rmsnorm_model.py.

selector   N = K, row r has code 1 in column r and code 0 elsewhere, lut[r] = [0, 1, 0, ...] (`norm_selector`).  The constant Moebius
           coefficient (plane_core.h:3-6) is lut[0] = 0 and the only non-zero bit-plane sum of row r is x_r, so y[r] is the normalised
           element itself on every family, the plane and stream kernels included (halfsweep_model.prologue_selector, code 0 on the
           diagonal and 1 = lut[0], would make y a difference of K-long sums there).  -0 arrives as +0: zeros compare by value.
           gq_dense_gemv_f16 takes the K x K identity.  K = 2048 (4096 for pair-table), the lowest bit width the family serves.
inputs     rmsnorm_model.banded / interleaved / gauss, eps 1e-5 and 1e-6, weights without powers of two in +-[0.5, 2).  The plane and
           stream families run banded and gauss only: their contract allows loss below 2^-17 of the vector's maximum
           (plane_core.h:104-108), and an interleaved vector has outputs of 2^-24 next to outputs of order ten.
reach      the plain launch on the same route, fed the model's primary output vector, must return it bit for bit: then the normalised
           vector can be seen element by element.  rmsnorm_model.reachable bounds the dynamic range of a vector on the CPU first; a
           vector it rejects is not launched (counted and printed; tests/test_rmsnorm_model_cpu.py asserts that nearly all pass and
           that every fault is still caught on those that do).
q/k/v      H * hd = K = 2048 (32 heads of 64), 8 KV heads whose rows are all code 0 (k = v = 0), position 0, the cos table all ones
           and the sin table all zeros: q is the normalised vector by value.  The launch has no form without the norm; the reach check
           is the stream family's plain launch, which builds the same activation image.
The last test prints, per site: draws, outputs that were not the primary candidate, the multi-candidate share, subnormal and zero
outputs seen.  The interleaved runs must see both subnormals and zeros (asserted).

Measured on an MI355X -- no value outside its candidates, no vector rejected by `reachable`, every plain launch returned the primary
vector bit for bit (both eps and the family's arrangements together):
  site         draws     non-primary   two candidates   subnormal outputs   zero outputs   grant
  exact        303 104   12            0.38 %           44 154              13 396         2^-19.31
  wide         303 104   12            0.38 %           44 154              13 396         2^-19.31
  pair-table   360 448   67            0.51 %           44 209              21 508         2^-18.61
  dq           303 104    8            0.38 %           44 154              13 396         2^-19.31
  plane        176 128    2            0.55 %               10                   4         2^-19.06
  stream       176 128    2            0.42 %               10                   4         2^-19.50
  stream-ho    176 128    2            0.29 %               10                   4         2^-20.03
  qkv-rope     176 128    2            0.42 %               10                   4         2^-19.50
  dense        303 104    2            0.24 %           44 154              13 396         2^-19.99
(exact and wide share rms_scale and its item order: the same figures.  The plane and stream families see subnormal outputs only in the
first banded row and in a few Gaussian elements: the interleaved rows are not theirs.)
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import halfsweep_model as hs  # noqa: E402
import rmsnorm_model as rm  # noqa: E402
import test_bounds_ap_gemv_gpu as t  # noqa: E402
from ap_helpers import assert_route, run_fused_guarded  # noqa: E402
from test_bounds_ap_gemv_gpu import _restore_env  # noqa: E402,F401  (autouse: the GQ_* environment and the mode are put back)

STATS = {}
# family -> (K, arrangements)
FAMILIES = {"exact": (2048, ("banded", "interleaved", "gauss")), "pair-table": (4096, ("banded", "interleaved", "gauss")),
            "wide": (2048, ("banded", "interleaved", "gauss")), "dq": (2048, ("banded", "interleaved", "gauss")),
            "plane": (2048, ("banded", "gauss")), "stream": (2048, ("banded", "gauss"))}


def lowest_bits(fam):
    """the lowest bit width among the CASES rows of the family that list the norm form"""
    return min(bits for f, bits, _, _, forms, _ in t.CASES if f == fam and "norm" in forms)


def norm_selector(K, bits, rows=None):
    """(qweight, lut): `rows` (default K) rows, row r < K with code 1 in column r only, lut[r] = [0, 1, 0, ...]: y[r] = x_r, y[r >= K] = 0"""
    codes = np.zeros((rows or K, K), dtype=np.uint8)
    codes[np.arange(K), np.arange(K)] = 1
    q, lut = hs._selector(codes, bits, 0.0)
    lut[:, 1] = 1.0
    return q, lut


def _record(site, arr, out, cand, what):
    ok, npri = hs.in_candidates(out, cand, zero_signs=False)
    bad = np.argwhere(~ok)
    _, _, nmulti, nsub, nzero = rm.tally(out, cand)
    s = STATS.setdefault(site, [0, 0, 0, 0, 0])
    for i, v in enumerate((out.size, int(npri.sum()), nmulti, nsub, nzero)):
        s[i] += v
    print(f"{site} {what} {arr}: {out.size} draws, {int(npri.sum())} non-primary, {nmulti} with two candidates, {nsub} subnormal, {nzero} zero outputs")
    assert bad.shape[0] == 0, "%s %s %s: %d outputs outside their candidates; (index, got, lower, primary, upper) bits: %s" % (
        site, what, arr, bad.shape[0], [(tuple(i), ) + tuple(hex(hs.bits(a)[tuple(i)]) for a in (out, cand[0], cand[1], cand[2])) for i in bad[:6]])
    if arr == "interleaved":
        assert nsub > 0 and nzero > 0, (nsub, nzero)


def _sweep(site, fam, arr, K, launch_plain, launch_norm):
    """every vector of the arrangement through launch_norm(x, w, eps) -> y[K], after launch_plain(primary) -> y[K] returned the primary
    output bit for bit (-0 as +0)"""
    x, w = rm.ARRANGEMENTS[arr](K), rm.weights(K)
    for eps in rm.EPSS:
        cand = rm.candidates(x, w, eps, K, site)
        keep = [r for r in range(x.shape[0]) if rm.reachable(cand[1][r], fam)]
        assert len(keep) >= 0.9 * x.shape[0] or arr == "gauss" and len(keep) >= 0.5 * x.shape[0], (len(keep), x.shape[0])
        got = np.zeros((len(keep), K), dtype=np.float16)
        for i, r in enumerate(keep):
            plain = launch_plain(cand[1][r])
            arrived = hs.same(plain, cand[1][r], zero_signs=False)
            assert arrived.all(), "%s %s row %d: the plain launch does not return %d elements of the primary vector; (sent, got) bits: %s" % (
                site, arr, r, int((~arrived).sum()), [(hex(hs.bits(cand[1][r])[j]), hex(hs.bits(plain)[j])) for j in np.flatnonzero(~arrived)[:6]])
            got[i] = launch_norm(x[r], w, eps)
        _record(site, arr, got, cand[:, keep], f"K {K} eps {eps} ({x.shape[0] - len(keep)} vectors not reachable)")


# ------------------------------------------------------------------------------------------------ gq_anyprec_gemv_fused, family by family
@pytest.mark.parametrize("fam,arr", [(f, a) for f in sorted(FAMILIES) for a in FAMILIES[f][1]])
def test_rmsnorm_prologue_family(fam, arr):
    from guidedquant_amd import _lib
    K, bits = FAMILIES[fam][0], lowest_bits(fam)
    t.set_env(fam)
    for has_norm in (False, True):
        assert _lib.ap_plan_route(K, K, bits, 1, has_norm, 0, 0)[0] == fam
    q, lut = norm_selector(K, bits)
    _sweep(fam, fam, arr, K, lambda v: run_fused_guarded(v, q, lut, bits, expect=fam),
           lambda x, w, eps: run_fused_guarded(x, q, lut, bits, norm_weight=w, eps=eps, expect=fam))


# ------------------------------------------------------------------------------------------------ the stream kernel's hand-over form
@pytest.mark.parametrize("arr", ["banded", "gauss"])
def test_rmsnorm_prologue_stream_with_handed_over_statistics(arr):
    from guidedquant_amd import _lib
    L = _lib.lib()
    K, bits, d = 2048, lowest_bits("stream"), torch.device("cuda:0")
    t.set_env("stream")
    assert L.gq_anyprec_handover_plan(K, K, bits, 1, 0) & 1, "the stream kernel's RMSNorm prologue takes the statistics at this shape"
    q, lut = norm_selector(K, bits)
    qt, lt = torch.from_numpy(q).to(d), torch.from_numpy(lut).to(d)

    def launch_norm(x, w, eps):
        xt, wt = torch.from_numpy(np.ascontiguousarray(x)).to(d), torch.from_numpy(w).to(d)
        ssq = torch.full((_lib.SSQ_SLOTS, ), float("nan"), dtype=torch.float32, device=d)
        _lib.check(L.gq_ssq_rows(xt.data_ptr(), K, ssq.data_ptr(), _lib.current_stream_ptr()), "gq_ssq_rows")
        out = torch.full((K, ), float("nan"), dtype=torch.float16, device=d)
        _lib.check(L.gq_anyprec_gemv_fused_ho(xt.data_ptr(), out.data_ptr(), qt.data_ptr(), lt.data_ptr(), K, K, bits, wt.data_ptr(), eps, None, 0, None, 0,
                                              ssq.data_ptr(), None, _lib.current_stream_ptr()), "gq_anyprec_gemv_fused_ho")
        assert_route("stream")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    _sweep("stream-ho", "stream", arr, K, lambda v: run_fused_guarded(v, q, lut, bits, expect="stream"), launch_norm)


# ------------------------------------------------------------------------------------------------ gq_anyprec_gemv_qkv_rope
@pytest.mark.parametrize("arr", ["banded", "gauss"])
def test_rmsnorm_prologue_of_the_fused_qkv_launch(arr):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv, hd, K, bits, MS, d = 32, 8, 64, 2048, 2, 4, torch.device("cuda:0")
    N = (H + 2 * Hkv) * hd
    t.set_env("stream")
    assert L.gq_anyprec_qkv_rope_supported(N, K, bits, hd), "the fused q/k/v launch serves the 1B attention geometry"
    q, lut = norm_selector(K, bits, rows=N)
    qs, luts = norm_selector(K, bits)
    qt, lt = torch.from_numpy(q).to(d), torch.from_numpy(lut).to(d)
    cos, sin = torch.ones(MS, hd, dtype=torch.float16, device=d), torch.zeros(MS, hd, dtype=torch.float16, device=d)
    pos = torch.zeros(1, dtype=torch.int32, device=d)

    def launch_norm(x, w, eps):
        xt, wt = torch.from_numpy(np.ascontiguousarray(x)).to(d), torch.from_numpy(w).to(d)
        out = torch.full((N, ), float("nan"), dtype=torch.float16, device=d)
        kc = torch.full((Hkv, MS, hd), float("nan"), dtype=torch.float16, device=d)
        vc = torch.full_like(kc, float("nan"))
        _lib.check(L.gq_anyprec_gemv_qkv_rope(xt.data_ptr(), out.data_ptr(), qt.data_ptr(), lt.data_ptr(), N, K, bits, wt.data_ptr(), eps, pos.data_ptr(),
                                              cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), H, Hkv, hd, MS, _lib.current_stream_ptr()),
                   "gq_anyprec_gemv_qkv_rope")
        torch.cuda.synchronize()
        assert not kc[:, 0].any() and not vc[:, 0].any() and torch.isnan(kc[:, 1:]).all() and torch.isnan(vc[:, 1:]).all()   # k = v = 0, at position 0 only
        return out[:K].cpu().numpy()

    _sweep("qkv-rope", "stream", arr, K, lambda v: run_fused_guarded(v, qs, luts, bits, expect="stream"), launch_norm)


# ------------------------------------------------------------------------------------------------ gq_dense_gemv_f16
@pytest.mark.parametrize("arr", ["banded", "interleaved", "gauss"])
def test_rmsnorm_prologue_of_the_dense_gemv(arr):
    from guidedquant_amd import _lib
    K, d = 2048, torch.device("cuda:0")
    W = torch.eye(K, dtype=torch.float16, device=d)

    def launch(x, w=None, eps=1e-5):
        xt = torch.from_numpy(np.ascontiguousarray(x)).to(d)
        wt = None if w is None else torch.from_numpy(w).to(d)
        out = torch.full((K, ), float("nan"), dtype=torch.float16, device=d)
        _lib.check(_lib.lib().gq_dense_gemv_f16(xt.data_ptr(), W.data_ptr(), out.data_ptr(), K, K, wt.data_ptr() if wt is not None else None, eps,
                                                _lib.current_stream_ptr()), "gq_dense_gemv_f16")
        torch.cuda.synchronize()
        return out.cpu().numpy()

    _sweep("dense", "dense", arr, K, launch, launch)


def test_print_the_tallies():
    """(last in the file) per site: draws, non-primary outputs, the multi-candidate share, subnormal and zero outputs seen"""
    for site, (n, npri, nmulti, nsub, nzero) in sorted(STATS.items()):
        print(f"{site}: {n} draws, {npri} non-primary, multi-candidate share {nmulti / n:.4f}, {nsub} subnormal and {nzero} zero outputs; grant 2^{math.log2(rm.grant(site)):.2f}")
        assert npri <= nmulti
