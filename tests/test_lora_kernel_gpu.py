"""GPU, kernel level: gq_lora_down + gq_lora_up (csrc/lora.hip) through the C ABI against a float64 host model of include/gq_hip.h's four
lines, xh of the normed site from tests/rmsnorm_model.py (its primary candidate: the contract's rounding points with rs = fp32(scale64)).

Bound per element: |out - ref64| <= ulp16(d64) + ulp16(out64): the two fp16 roundings at half an ulp each, doubled to cover the fp32 sums
(expected error sqrt(K) 2^-24).  The fp32 error is absolute -- about sqrt(r) 2^-24 x the largest term s B t, 2e-7 here -- so the bound needs
ulp16 of d or of out above it; without a base out = d, and those cases assert on the host, before the launch, that their seeded inputs
have no targeted |d64| below 2^-10 (ulp16 = 2^-20, four times the estimate).
Shapes: K 64 (one MFMA chunk) and 4096 + 64 (33 slices, a ragged last one); ranks 1, 16, 17 (padded 32), 64; N 16 and 6144 + 16 (a ragged
last row block); one and three segments, and q | - | v with an untargeted middle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rmsnorm_model as rm  # noqa: E402
from guarded import POISON, Guards, ptr  # noqa: E402

EPS = 1e-5
S = 2.0  # lora_alpha / r


def _ulp16(v):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0**-14)))
    return 2.0**(np.minimum(e, 15) - 10)


def _case(K, N, ranks, base, norm, seed=0):
    """ranks: one entry (one segment over all N rows) or three (rows N/2 | N/4 | the rest; 0: untargeted).  The kernels' inputs and ref64"""
    rng = np.random.default_rng(seed + K + N)
    x = rng.normal(0, 1, K).astype(np.float16)
    nw = rm.weights(K) if norm else None
    b16 = rng.normal(0, 1, N).astype(np.float16) if base else None
    cuts = [0, N] if len(ranks) == 1 else [0, N // 2, N // 2 + N // 4, N]
    xh = (rm.candidates(x[None], nw, EPS, K, "dense")[1][0] if norm else x).astype(np.float64)
    A, B, segs, d64 = [], [], [], np.zeros(N)
    for i, r in enumerate(ranks):
        if not r:
            continue
        rp, rows = (r + 15) // 16 * 16, cuts[i + 1] - cuts[i]
        a = np.zeros((rp, K), np.float16)
        b = np.zeros((rows, rp), np.float16)
        a[:r], b[:, :r] = rng.normal(0, K**-0.5, (r, K)), rng.normal(0, r**-0.5, (rows, r))
        segs.append((cuts[i], cuts[i + 1], sum(len(m) for m in A), rp, sum(m.size for m in B), S))
        A.append(a)
        B.append(b)
        d64[cuts[i]:cuts[i + 1]] = S * (b.astype(np.float64) @ (a.astype(np.float64) @ xh))
    out64 = d64 + b16.astype(np.float64) if base else d64
    return dict(x=x, nw=nw, base=b16, A=np.concatenate(A), B=np.concatenate([m.reshape(-1) for m in B]), segs=segs, K=K, N=N), d64, out64


def _launch(c, g=None, **over):
    """both launches on guard-banded buffers; (rc_down, rc_up, out fp16 [N] or None, guards).  `over`: arguments replaced for the refusals"""
    from guidedquant_amd import _lib
    L, sp = _lib.lib(), _lib.current_stream_ptr()
    g = g or Guards()
    R, K, N = over.get("R", len(c["A"])), over.get("K", c["K"]), c["N"]
    n = L.gq_lora_n_partials(c["K"])
    bufs = {k: g.inp(k, c[k]) for k in ("x", "nw", "A", "B", "base")}
    part, out = g.out("partials", n * len(c["A"]) * 4), g.out("out", N * 2)
    segs = over.get("segs", c["segs"])
    arr = (_lib.GqLoraSeg * len(segs))(*[_lib.GqLoraSeg(*s) for s in segs])
    rc_d = L.gq_lora_down(over.get("x", ptr(bufs["x"])), ptr(bufs["nw"]), EPS, ptr(bufs["A"]) + over.get("a_off", 0), R, K, part.ptr(), sp)
    rc_u = L.gq_lora_up(part.ptr(), n, R, ptr(bufs["B"]), arr, over.get("n_segs", len(segs)), ptr(bufs["base"]), out.ptr(), N, sp)
    g.check()
    return rc_d, rc_u, out.numpy(np.float16), g


@pytest.mark.parametrize("K,N,ranks,base,norm,seed", [
    (64, 16, (1, ), False, False, 0),
    (64, 16, (16, 1, 17), False, True, 0),
    (4096 + 64, 16, (64, ), True, True, 0),
    (64, 6144 + 16, (17, ), True, False, 0),
    (4096 + 64, 6144 + 16, (16, 0, 17), True, True, 0),
    (4096 + 64, 6144 + 16, (64, 64, 64), True, False, 0),
    (4096 + 64, 6144 + 16, (16, 0, 17), False, True, 5),
])
def test_lora_down_up_against_float64(K, N, ranks, base, norm, seed):
    c, d64, out64 = _case(K, N, ranks, base, norm, seed)
    assert base or np.abs(d64[d64 != 0]).min() >= 2.0**-10  # (the precondition of the bound where out = d)
    rc_d, rc_u, out, _ = _launch(c)
    assert (rc_d, rc_u) == (0, 0)
    err, bound = np.abs(out.astype(np.float64) - out64), _ulp16(d64) + _ulp16(out64)
    print(f"K={K} N={N} ranks={ranks}: max err / bound = {(err / bound).max():.3f}, max |d| = {np.abs(d64).max():.3f}")
    assert np.isfinite(out).all() and (err <= bound).all(), (int((err > bound).sum()), float((err / bound).max()))
    assert np.abs(d64).max() > 0.5  # (the delta is there to be got wrong)
    _, _, again, _ = _launch(c)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16))  # (fixed-order sums: a second launch is bit-equal)


@pytest.mark.parametrize("over,codes", [
    (dict(K=96), (-22, 0)), (dict(R=24), (-22, -22)), (dict(a_off=2), (-22, 0)), (dict(x=None), (-22, 0)), (dict(R=208), (-95, -95)),
    (dict(n_segs=4), (0, -22)), (dict(segs=[(0, 16, 0, 24, 0, S)]), (0, -22)), (dict(segs=[(0, 17, 0, 16, 0, S)]), (0, -22)),
    (dict(segs=[(8, 16, 0, 16, 0, S), (0, 8, 0, 16, 0, S)]), (0, -22)),
])
def test_lora_refusals_write_nothing(over, codes):
    c, _, _ = _case(128, 16, (16, ), True, True)
    rc_d, rc_u, _, g = _launch(c, **over)
    assert (rc_d, rc_u) == codes
    torch.cuda.synchronize()
    for name, rc in (("partials", rc_d), ("out", rc_u)):
        if rc:
            assert bool((g[name].view(torch.uint8) == POISON).all()), name
