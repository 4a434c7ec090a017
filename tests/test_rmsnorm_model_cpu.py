"""CPU: the host model of the RMSNorm sweeps (tests/rmsnorm_model.py) against independent statements of the contract, its strictness,
and its power to catch every injected fault in every site class on the inputs the GPU tests run.  No device, no library."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halfsweep_model as hs  # noqa: E402
import rmsnorm_model as rm  # noqa: E402
from ap_helpers import rmsnorm_ref  # noqa: E402

CAP = 0.05   # at most this share of a case's elements may have more than one candidate: a condition, not a measurement


def _cases():
    for cls, (sites, arrs, Ds) in rm.CLASSES.items():
        for site in sites:
            for arr in arrs:
                for D in Ds:
                    if D <= rm.SITES[site]["D"]:   # (A was counted at the site's widest D)
                        yield site, arr, D


def test_grants_come_from_the_sites_and_stay_small():
    for site, s in rm.SITES.items():
        g = rm.grant(site)
        assert g == ((s["A"] + 1) * 2.0**-24 * 1.01 + 2 * 2.0**-24) / 2 + 2.0**-23
        assert 2.0**-23 < g < 2.0**-18, (site, np.log2(g))   # far below an fp16 step (2^-11): one or two candidates
        assert s["where"] and s["expr"] in ("rsqrtf", "1/sqrtf")
    assert set(s for c in rm.CLASSES.values() for s in c[0]) == set(rm.SITES)


def test_arrangements_and_weights():
    for D in (8, 64, 128, 520, 2048, 4096, 16384):
        b, i = rm.banded(D), rm.interleaved(D)
        for a in (b, i):
            assert a.shape[1] == D and a.size - hs.FINITE.size < D
            assert np.array_equal(np.unique(hs.bits(a)), np.unique(hs.FINITE))   # every finite pattern (the padding repeats +0)
        mag = np.abs(b.astype(np.float64))
        assert (np.diff(mag.reshape(-1)) >= 0).all()
        if D <= 2048:   # a row of the banded order: two binades at most, subnormal row aside
            lo = np.where(mag > 0, mag, np.inf).min(axis=1)
            rows = lo >= 2.0**-14
            assert (mag.max(axis=1)[rows] < 4 * lo[rows]).all()
        w = rm.weights(D)
        assert ((hs.bits(w) & 0x3FF) != 0).all() and (np.abs(w) >= 0.5).all() and (np.abs(w) < 2).all() and (w < 0).any() and (w > 0).any()
        d = rm.delta_for(b)
        assert np.isfinite((b.astype(np.float32) + d.astype(np.float32)).astype(np.float16)).all() and (d != 0).any()


@pytest.mark.parametrize("eps", rm.EPSS)
@pytest.mark.parametrize("D", [8, 64, 520, 2048, 16384])
def test_banded_rows_reach_the_eps_regime_and_interleaved_rows_the_subnormals(D, eps):
    w = rm.weights(D)
    s = rm.scale64(rm.banded(D), eps, D)
    # eps alone sets the scale of the tiny rows, the largest rows have ~1.5e-5 (at D = 16384 a row is eight binades: eps still has a
    # half in the first one, and the last one's scale is that of its upper binades)
    assert s.max() > (0.99 if D <= 2048 else 0.5) / np.sqrt(eps) and s.min() < (2.5e-5 if D <= 2048 else 1e-4)
    out = rm.candidates(rm.interleaved(D), w, eps, D, "rows")[1]
    sub, zero = ((out != 0) & (np.abs(out) < 2.0**-14)).mean(), (out == 0).mean()
    print(f"interleaved D {D} eps {eps}: {sub:.3f} subnormal outputs, {zero:.3f} zeros")
    assert sub >= 0.25 and zero >= 0.05, (sub, zero)   # about a third and a tenth
    xi = rm.interleaved(D)   # ... and behind the residual add in front
    out = rm.candidates((xi.astype(np.float32) + rm.delta_for(xi).astype(np.float32)).astype(np.float16), w, eps, D, "rows")[1]
    assert ((out != 0) & (np.abs(out) < 2.0**-14)).mean() >= 0.25 and (out == 0).mean() >= 0.05


@pytest.mark.parametrize("eps", rm.EPSS)
@pytest.mark.parametrize("D", [64, 128, 520, 2048, 4096])
def test_primary_candidate_is_the_reference_rounding_and_the_torch_expression(D, eps):
    x, w = rm.gauss(D, rows=8), rm.weights(D)
    cand = rm.candidates(x, w, eps, D, "rows")
    ref = np.stack([rmsnorm_ref(r, w, eps) for r in x])
    assert hs.same(cand[1], ref).all(), "the primary candidate is ap_helpers.rmsnorm_ref bit for bit"
    xt, wt = torch.from_numpy(x.copy()), torch.from_numpy(w.copy())
    t = ((xt.float() * torch.rsqrt(xt.float().pow(2).mean(-1, keepdim=True) + eps)).half() * wt).numpy()
    ok, npri = hs.in_candidates(t, cand)
    print(f"torch on the CPU, D {D} eps {eps}: {int(npri.sum())} of {t.size} outputs are not the primary candidate")
    assert ok.all(), "torch's fp32 expression (its own summation order) stays within the candidates"
    assert npri.sum() <= rm.multi(cand).sum()


@pytest.mark.parametrize("site,arr,D", sorted(set(_cases())))
def test_at_most_a_twentieth_of_the_elements_have_two_candidates(site, arr, D):
    x, w = rm.ARRANGEMENTS[arr](D), rm.weights(D)
    for eps in rm.EPSS:
        share = rm.multi(rm.candidates(x, w, eps, D, site)).mean()
        assert share <= CAP, (site, arr, D, eps, share)


def _gpu_vectors(cls, arr, D, eps):
    """the rows of an arrangement the GPU test of a class checks: all of them, or for the plane / stream GEMVs those both can carry"""
    x, w = rm.ARRANGEMENTS[arr](D), rm.weights(D)
    if cls != "gemv plane / stream":
        return x, w
    pri = rm.candidates(x, w, eps, D, "plane")[1]
    keep = [r for r in range(x.shape[0]) if rm.reachable(pri[r], "plane") and rm.reachable(pri[r], "stream")]
    return x[keep], w


@pytest.mark.parametrize("fault", rm.FAULTS)
@pytest.mark.parametrize("cls", sorted(rm.CLASSES))
def test_every_fault_is_caught_in_every_site_class(cls, fault):
    sites, arrs, Ds = rm.CLASSES[cls]
    D = max(Ds)
    for site in sites:
        if D > rm.SITES[site]["D"]:
            continue
        caught = {}
        for arr in arrs:
            for eps in rm.EPSS:
                x, w = _gpu_vectors(cls, arr, D, eps)
                ok, _ = hs.in_candidates(rm.faulty(fault, x, w, eps, D), rm.candidates(x, w, eps, D, site), zero_signs=False)
                caught[arr, eps] = int((~ok).sum())
        print(f"{cls} / {site} / {fault}: elements outside their candidates {caught}")
        assert max(caught.values()) > 0, (cls, site, fault)


def test_the_plane_and_stream_kernels_can_carry_the_vectors_they_are_given():
    """banded and gauss outputs are of order one: nearly every vector passes the bound of rmsnorm_model.reachable; the interleaved
    ones (outputs down to 2^-24 next to outputs of order ten) do not, which is why those families do not run them"""
    D, w = 2048, rm.weights(2048)
    for eps in rm.EPSS:
        for arr, least in (("banded", 0.9), ("gauss", 0.5)):
            pri = rm.candidates(rm.ARRANGEMENTS[arr](D), w, eps, D, "plane")[1]
            for fam in ("plane", "stream"):
                share = np.mean([rm.reachable(v, fam) for v in pri])
                print(f"{arr} eps {eps} {fam}: {share:.2f} of the vectors reachable")
                assert share >= least, (arr, eps, fam, share)
        pri = rm.candidates(rm.interleaved(D), w, eps, D, "plane")[1]
        assert not any(rm.reachable(v, "stream") for v in pri)
