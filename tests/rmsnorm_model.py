"""Host model of the RMSNorm sweeps (tests/test_rmsnorm_rows_gpu.py, tests/test_rmsnorm_ap_gpu.py): what every RMSNorm site of the serving
paths may write for a row of fp16 values.  Plain numpy, float64, no device, no library.  Like tests/halfsweep_model.py it restates the
CONTRACT (inference/model.py:281-292), not the kernels:

    n = fp16(fp32(float(x) * rs)),  rs = rsqrt(mean(x^2) + eps) in fp32;      out = fp16(n * w)         -- two fp16 roundings, fp32 between

`scale64`     1 / sqrt(sum(x^2) / D + eps) in float64: what rs approximates.
`grant`       the relative interval around scale64 a site's fp32 rs may lie in, DERIVED FROM THE SITE'S CODE (SITES below: the longest
              addition path A of its sum of squares, next to the file:line it was counted at), never from its outputs:
                a sum of non-negative fp32 terms (the squares of fp16 values are exact in fp32) whose longest path has A additions is
                within (A + 1) 2^-24 * 1.01 relative of the true sum; two more roundings for `/ D` and `+ eps`; half of the total for
                the square root; 2^-23 for the rsqrtf or 1.0f / sqrtf expression (the library is built without fast-math: sqrtf and
                the division are correctly rounded, rsqrtf is within an ulp).
              The entries take eps as an fp32, and 1e-5 and 1e-6 are not fp32 values: the interval is laid around scale64 at the
              double AND at its fp32 rounding (2.5e-8 apart at most, in the eps-dominated rows), not widened by a term of the grant.
              A v_dot2_f32_f16 step (the stream kernel's spelling of two squares and an add) is counted as two additions.
`candidates`  fp32(x * rs) is monotone in rs, so the admissible n of an element are the fp16 values between the roundings at the two
              ends of the interval -- one or two neighbouring values (asserted) -- and the admissible outputs are fp16(n * w) of each.
              Returned as [3, ...]: the output at the lower end, the PRIMARY candidate (rs = fp32(scale64): ap_helpers.rmsnorm_ref
              bit for bit) and the output at the upper end, the layout halfsweep_model.in_candidates takes.
comparison    by bit pattern (halfsweep_model.same); -0 and +0 compare equal only where the site's arithmetic cannot fix the sign:
              behind a GEMV's sum and behind the rotation x * 1 + (-+y) * 0 of the QK-norm sites (zero_signs=False there).
arrangements  of halfsweep_model.FINITE, the 63 488 finite patterns, padded with zeros to a multiple of D (`banded`, `interleaved`), and
              seeded Gaussians (`gauss`); `weights` are seeded, finite, no powers of two, magnitudes in [0.5, 2), both signs: the second
              rounding is real everywhere and nothing overflows (|n| <= sqrt(D) <= 128).
`reachable`   which vectors the plane / stream GEMV can carry element by element (plane_core.h:104-116): decided on the CPU, from the
              kernels' stated scaling rule, before anything is launched.
`faulty`      the primary output with exactly one deviation from the contract, for tests/test_rmsnorm_model_cpu.py only.
"""
import numpy as np

import halfsweep_model as hs

EPSS = (1e-5, 1e-6)
GAUSS_SCALES = (2.0**-12, 1.0, 2.0**10)
FAULTS = ("no_eps", "wrong_divisor", "one_rounding", "flush_n", "flush_out", "truncate", "fp16_scale")

# site -> A, the longest addition path of its sum of squares at the widest D its test uses (an upper bound where the launch plan
# decides the exact number), and where it was read.  per-thread chain + the 6 steps of a 64-lane tree + the cross-wave adds.
SITES = {
    # csrc/prefill.hip:42-63 a thread adds 8 units x 8 squares (D = 16384); :65 wave_sum, 6 steps; :68 red[0] + red[1] + red[2] + red[3]
    "rows": dict(A=64 + 6 + 3, D=16384, where="csrc/prefill.hip:42-68", expr="rsqrtf"),
    # csrc/ap_exact.h:106-126 a stager thread adds 32 squares per item; the stagers are at least one wave (ap_gemv.hip:142, :279,
    # ap_wide.hip:94: T >= 64), K / 32 items: one item each at K = 2048, two at 4096; :127 wave_allsum, 6 steps; :131 wave_allsum again
    "exact": dict(A=32 + 6 + 6, D=2048, where="csrc/ap_exact.h:106-132", expr="1/sqrtf"),
    "wide": dict(A=32 + 6 + 6, D=2048, where="csrc/ap_exact.h:106-132 (ap_wide.hip:94)", expr="1/sqrtf"),
    "pair-table": dict(A=64 + 6 + 6, D=4096, where="csrc/ap_exact.h:106-132 (ap_gemv.hip:279)", expr="1/sqrtf"),
    "dq": dict(A=32 + 6 + 6, D=2048, where="csrc/ap_exact.h:106-132 (ap_dq.hip:193: DQ_WAVES / 2 stager waves)", expr="1/sqrtf"),
    # csrc/ap_plane.hip:660-664 two adds per packed pair, 4 pairs per unit, NI units per early-wave thread (K / 8 = 256 units over
    # E * 64 threads: NI <= 4); :707 wave_reduce_l63, 6 steps; :730 the E <= 16 early waves' sums one after the other
    "plane": dict(A=32 + 6 + 16, D=2048, where="csrc/ap_plane.hip:660-664, :707, :728-731 (detect(): :611-614, the same sums)", expr="1/sqrtf"),
    # csrc/ap_stream.hip:441-444 NPU <= 2 units (:1114, :1143: NPU = 4 serves no RMSNorm) x 4 v_dot2 (2 additions each); :445 the tree;
    # :462 the W <= 16 builder waves' sums one after the other
    "stream": dict(A=16 + 6 + 16, D=2048, where="csrc/ap_stream.hip:441-445, :460-463", expr="1/sqrtf"),
    # the hand-over form: producer csrc/ap_dispatch.hip:22-25 slot t adds elements t, t + 1024 (K = 2048: 2 terms); consumer
    # csrc/ap_stream.hip:311-321 4 x 4 slots per lane, then the tree
    "stream-ho": dict(A=2 + 16 + 6, D=2048, where="csrc/ap_dispatch.hip:22-25 + csrc/ap_stream.hip:311-322", expr="1/sqrtf"),
    # the stream kernel's instance compiled for gq_anyprec_gemv_qkv_rope (ap_stream.hip:1237: NPU = 1, W = ST_W2)
    "qkv-rope": dict(A=16 + 6 + 16, D=2048, where="csrc/ap_stream.hip:441-445, :460-463 (:1237)", expr="1/sqrtf"),
    # csrc/decode.hip:620-650 a thread adds its units of 8 squares (K / 8 = 256 units over 256 threads, at most 2 kept: 16); :651 the
    # tree; :654 red[0] + red[1] + red[2] + red[3]
    "dense": dict(A=16 + 6 + 3, D=2048, where="csrc/decode.hip:620-654", expr="1/sqrtf"),
    # csrc/prefill.hip:243-254 a thread adds 16 squares, then log2(hd / 16) <= 3 butterfly steps
    "qkn-rows": dict(A=16 + 3, D=128, where="csrc/prefill.hip:243-254, :267", expr="rsqrtf"),
    # csrc/decode.hip:237-246 one square per thread, the tree, the two waves' sums added from 0 (hd = 128)
    "qkn-decode": dict(A=6 + 2, D=128, where="csrc/decode.hip:237-246", expr="rsqrtf"),
}
# the classes a fault must be caught in: (sites, arrangements their GPU test runs, (D, ..))
CLASSES = {
    "rows": (("rows", ), ("banded", "interleaved", "gauss"), (8, 520, 2048, 16384)),
    "gemv exact-order + dq": (("exact", "wide", "dq"), ("banded", "interleaved", "gauss"), (2048, )),
    "gemv pair-table": (("pair-table", ), ("banded", "interleaved", "gauss"), (4096, )),
    "gemv plane / stream": (("plane", "stream", "stream-ho", "qkv-rope"), ("banded", "gauss"), (2048, )),
    "dense": (("dense", ), ("banded", "interleaved", "gauss"), (2048, )),
    "qk-norm": (("qkn-rows", "qkn-decode"), ("banded", "interleaved"), (64, 128)),
}


def grant(site):
    """the relative half-width of the interval around scale64 the site's fp32 scale lies in"""
    A = SITES[site]["A"]
    return ((A + 1) * 2.0**-24 * 1.01 + 2 * 2.0**-24) / 2 + 2.0**-23


def scale64(x16, eps, D):
    """1 / sqrt(sum(x^2) / D + eps) in float64, per row of x16 [R, D] -> [R, 1] (the squares and, at these sizes, their sum are exact)"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64).reshape(-1, D)
    return 1.0 / np.sqrt((x * x).sum(axis=1, keepdims=True) / D + np.float64(eps))


def _norm(x64, rs32, w64=None):
    """fp16(fp32(x * rs)) for an fp32-valued rs (the 11 x 24 bit product is exact in float64: one rounding to fp32, one to fp16); with
    w64 the output fp16(n * w) (exact product of two halves, one rounding)"""
    n = (x64 * rs32.astype(np.float64)).astype(np.float32).astype(np.float16)
    return n if w64 is None else hs.to_half(n.astype(np.float64) * w64)


def _ends(s_lo, s_hi, g):
    """the fp32 values that enclose [s_lo (1 - g), s_hi (1 + g)]: rounded outwards"""
    lo, hi = s_lo * (1.0 - g), s_hi * (1.0 + g)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32, hi32


def candidates(x16, w16, eps, D, site):
    """fp16 [3, R, D]: the outputs at the lower end of the site's interval, at fp32(scale64) (the primary candidate) and at the upper end.
    Every admissible output is one of rows 0 and 2: the n of the two ends are equal or fp16 neighbours (asserted), and the primary n,
    which lies between them, is one of the two."""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64).reshape(-1, D)
    w = np.asarray(w16, dtype=np.float16).astype(np.float64).reshape(1, D)
    s, s32 = scale64(x16, eps, D), scale64(x16, np.float64(np.float32(eps)), D)   # (eps as the contract's double, and as the entry's fp32)
    lo32, hi32 = _ends(np.minimum(s, s32), np.maximum(s, s32), grant(site))
    n = [_norm(x, r) for r in (lo32, s.astype(np.float32), hi32)]
    a, b = np.minimum(n[0], n[2]), np.maximum(n[0], n[2])   # (negative x: the order turns round)
    assert ((a == b) | (np.nextafter(a, np.float16(np.inf)) == b)).all(), "an interval wider than an fp16 step"
    assert (hs.same(n[1], n[0]) | hs.same(n[1], n[2])).all()
    return np.stack([hs.to_half(c.astype(np.float64) * w) for c in n])


def multi(cand):
    """element-wise: more than one admissible output"""
    return ~hs.same(cand[0], cand[2])


# ------------------------------------------------------------------------------------------------ inputs
def _pad(patterns, D):
    n = -(-patterns.size // D) * D
    return np.concatenate([np.zeros(n - patterns.size, dtype=np.uint16), patterns])


def banded(D):
    """fp16 [R, D]: the finite patterns in the order of their magnitudes (+x next to -x), the padding zeros in front: a row spans two
    binades at most.  The tiny rows are eps-dominated (scale up to 1 / sqrt(eps)), the large ones have scales down to 1.5e-5."""
    order = np.argsort(hs.FINITE & 0x7FFF, kind="stable")
    return hs.half(_pad(hs.FINITE[order], D)).reshape(-1, D)


def interleaved(D):
    """fp16 [R, D]: row r takes every R-th pattern of the banded order: each row strides over the whole range, its largest elements set
    the scale and most of the others become fp16 subnormals or zeros"""
    b = banded(D)
    return np.ascontiguousarray(b.reshape(D, -1).T)


def gauss(D, rows=4, seed=11):
    """fp16 [3 * rows, D]: N(0, 1) * s for s = 2^-12 (eps-dominated), 1 and 2^10, `rows` rows each"""
    rng = np.random.default_rng(seed + D)
    return np.concatenate([(rng.normal(0, 1, (rows, D)) * s).astype(np.float16) for s in GAUSS_SCALES])


ARRANGEMENTS = {"banded": banded, "interleaved": interleaved, "gauss": gauss}


def weights(D, seed=5):
    """fp16 [D]: magnitudes in [0.5, 2), no powers of two, both signs"""
    rng = np.random.default_rng(seed + D)
    m = rng.uniform(0.5, 2.0, D).astype(np.float16)
    m = np.where((hs.bits(m) & 0x3FF) == 0, np.nextafter(m, np.float16(1.5)), m).astype(np.float16)
    m = np.clip(m, np.float16(0.5), np.nextafter(np.float16(2), np.float16(0)))
    assert ((hs.bits(m) & 0x3FF) != 0).all() and (m >= 0.5).all() and (m < 2).all()
    return (m * rng.choice([-1.0, 1.0], D)).astype(np.float16)


def delta_for(x16, seed=3):
    """a residual delta for which no x + delta overflows and which leaves an arrangement its ranges: element by element a random
    fraction in [0.25, 0.75) of |x| (x + delta is a real fp16 rounding), of a random sign unless the magnitudes would add up beyond the
    largest finite value -- then of the opposite sign to x.  A zero stays a zero."""
    x = np.asarray(x16, dtype=np.float16)
    rng = np.random.default_rng(seed + x.shape[-1])
    mag = np.abs(x.astype(np.float64)) * rng.uniform(0.25, 0.75, x.shape)
    sign = rng.choice([-1.0, 1.0], x.shape)
    sign = np.where(np.abs(x.astype(np.float64)) + mag >= 65504.0, -np.copysign(1.0, x.astype(np.float64)), sign)
    d = hs.to_half(mag * sign)
    assert np.isfinite((x.astype(np.float32) + d.astype(np.float32)).astype(np.float16)).all()
    return d


# ------------------------------------------------------------------------------------------------ what a plane / stream GEMV can carry
def _lsb(v16):
    """the value of the lowest set bit of each fp16 value (inf for a zero)"""
    b = hs.bits(v16).astype(np.int64).reshape(np.shape(v16))
    e, m = (b >> 10) & 0x1F, b & 0x3FF
    sig = np.where(e > 0, m | 0x400, m)
    low = sig & -sig
    with np.errstate(divide="ignore"):
        return np.where(sig == 0, np.inf, low.astype(np.float64) * 2.0**(np.maximum(e, 1) - 25))


def _shift(bound):
    """plane_core.h:109-115 piece_shift of an upper bound of max |x|"""
    with np.errstate(divide="ignore"):
        eb = np.where(bound > 0, np.floor(np.log2(np.maximum(bound, 1e-300))) + 1, 15)
    return np.clip(15 - eb, -14, 15)


def reachable(v16, family):
    """whether a plane / stream GEMV carries every element of the activation vector v16 [K] exactly (plane_core.h:104-108): the vector
    is multiplied by 2^k, k = piece_shift(an upper bound U of its maximum), and split into four bf8 pieces; a piece below the bf8
    normals (2^-14) is not carried exactly.  So every set bit of v * 2^k must be worth 2^-14 at least.  U, generously:
      plane   the maximum, times 1.002 and the roundings of the bound (ap_plane.hip:732): twice the maximum covers it;
      stream  per unit of the image (512 activations: ap_stream.hip:331) the extraction threshold, 64 * 1.01 x the unit's mean magnitude
              rounded up to fp16 (ap_stream.hip:500-506): 66 x the largest mean of any aligned 128 of the vector covers every unit;
              elements above it leave the image and are multiplied on their own.
    The other families sum fp32 products of fp16 values: one non-zero product per row, exact."""
    v = np.abs(np.asarray(v16, dtype=np.float16).astype(np.float64)).reshape(-1)
    if family not in ("plane", "stream"):
        return True
    if family == "plane":
        k = _shift(2.0 * v.max())
    else:
        k = _shift(np.maximum(66.0 * v.reshape(-1, 128).mean(axis=1).max(), 2.0**-24))
    return bool((_lsb(v16).reshape(-1) * 2.0**k >= 2.0**-14).all())


# ------------------------------------------------------------------------------------------------ injected faults
def faulty(fault, x16, w16, eps, D):
    """the primary output [R, D] with exactly one deviation from the contract"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float64).reshape(-1, D)
    w = np.asarray(w16, dtype=np.float16).astype(np.float64).reshape(1, D)
    ssq = (x * x).sum(axis=1, keepdims=True)
    s = scale64(x16, eps, D)
    if fault == "no_eps":
        s = np.where(ssq > 0, 1.0 / np.sqrt(np.where(ssq > 0, ssq, 1.0) / D), s)
    elif fault == "wrong_divisor":   # the mean over the next power of two
        s = 1.0 / np.sqrt(ssq / 2.0**int(np.floor(np.log2(D)) + 1) + np.float64(eps))
    elif fault == "fp16_scale":
        s = hs.to_half(s).astype(np.float64)
    rs = np.minimum(s, 3.0e38).astype(np.float32)
    if fault == "one_rounding":
        return hs.to_half((x * rs.astype(np.float64)).astype(np.float32).astype(np.float64) * w)
    n = _norm(x, rs)
    if fault == "truncate":   # round towards zero in the first conversion
        p = (x * rs.astype(np.float64)).astype(np.float32)
        n = np.where(np.abs(n.astype(np.float32)) > np.abs(p), np.nextafter(n, np.float16(0)), n).astype(np.float16)
    if fault == "flush_n":
        n = np.where(np.abs(n) < 2.0**-14, np.copysign(np.float16(0), n), n).astype(np.float16)
    out = hs.to_half(n.astype(np.float64) * w)
    if fault == "flush_out":
        out = np.where(np.abs(out) < 2.0**-14, np.copysign(np.float16(0), out), out).astype(np.float16)
    assert fault in FAULTS, fault
    return out


def tally(out16, cand):
    """(all within the candidates?, non-primary outputs, multi-candidate elements, subnormal outputs, zero outputs) with signs of zeros
    left to the caller (`ok` here is by value for zeros)"""
    ok, npri = hs.in_candidates(out16, cand, zero_signs=False)
    o = np.asarray(out16, dtype=np.float16)
    return ok, int(npri.sum()), int(multi(cand).sum()), int(((o != 0) & (np.abs(o) < 2.0**-14)).sum()), int((o == 0).sum())
