"""Host model of the full-domain sweeps (tests/test_halfsweep_rows_gpu.py, tests/test_halfsweep_ap_gpu.py): what every one of the 65 536
fp16 bit patterns must become behind the two per-element rounding points on every token's path, SiLU * up and the fp8 (e4m3) cache
write.  numpy and torch on the CPU: no GPU, no library.  Like tests/sampler_lp_model.py it restates the CONTRACT, not the kernels.

SiLU * up     q = g / (1 + e^-g) in float64.  A device evaluates q in fp32 with a relative error of at most `delta`; the fp16 SiLU is
              then one of fp16(q (1 - delta)), fp16(q), fp16(q (1 + delta)) (`silu_candidates`; rounding is monotone, and over the
              whole domain the outer two are never more than one ulp apart, so the three are every value in between), and the output
              is fp16(float64(c) * float64(u)) for one of these c (`pair_candidates`: the product of two halves is exact in float64,
              one rounding).  A non-finite value compares by class (`same`): NaN is NaN, Inf is Inf with its sign; zeros compare with
              their sign.
  DELTA_ROWS    2^-21, the expf site (gq_silu_mul_rows): one ulp of expf (2^-23 of e^-g, less of 1 + e^-g), the add and the correctly
                rounded division (2^-24 each) stay below 2^-22.6; the window leaves a factor of 3.
  DELTA_DECODE  2^-16, the __expf sites: test_ap_exact_fused_gpu.DELTA, whose derivation (|g| 2^-24 in the power, about an ulp each for
                v_exp_f32, the add and the division) holds to |g| <= 32.  Beyond it nothing is left to a window: for g > 32, e^-g < 2^-46
                and the fp32 quotient is g itself; below g = -20.4, |g e^g| < 2^-25 and the fp16 result is -0 under any relative error
                up to a half (the power's error, |g| 2^-24, stays below 2^-17 up to the |g| = 88.7 at which e^-g overflows to +Inf, and
                a finite g divided by +Inf is -0 again).
`scramble`    the fixed bijection of the 16-bit patterns that pairs gate i with another up in every row.
fp8 write     kv8_model.quantize, reused: code = fp8_rne(clamp(float(x16) * inv, -448, 448)); +-Inf clamps to +-448 (0x7e / 0xfe), a NaN
              stores a NaN code (0x7f or 0xff).  `fp8_ok` compares bytes under that rule; `fp8_ties` finds the inputs two codes are
              equally near to (at scale 1: the 252 midpoints of neighbouring codes and +-464, halfway to the 480 that has no code).
selectors     `pair_selector` / `prologue_selector`: Any-Precision layers whose GEMV copies planted fp16 values (or the SiLU * up
              prologue's products) into the output, so that an element-wise function inside a fused GEMV launch can be swept.
`FAULTS`      deviations `faulty_silu` / `faulty_fp8` inject into a correct output, for tests/test_halfsweep_model_cpu.py only.
"""
import numpy as np
import torch

import kv8_model as k8
from test_ap_exact_fused_gpu import DELTA as DELTA_DECODE  # (the value and its derivation live there)

DELTA_ROWS = 2.0**-21
PATTERNS = np.arange(65536, dtype=np.uint16)
FINITE = PATTERNS[(PATTERNS & 0x7C00) != 0x7C00]  # 63 488 of them
INV_SCALES = (1.0, 1 / 0.37, 1 / 2.9, 8.0)         # the reciprocal scales of the fp8 sweep on the CPU
SILU_FAULTS = ("subnormal_flush", "exp_2^-12", "neighbours_up", "no_fp16_silu")
FP8_FAULTS = ("truncate", "ties_away", "nan_beyond_448", "subnormal_codes_flushed", "nan_as_-448")
FAULTS = SILU_FAULTS + FP8_FAULTS


def half(bits):
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16)


def bits(h16):
    return np.ascontiguousarray(h16, dtype=np.float16).view(np.uint16)


def to_half(x64):
    """float64 -> fp16, one rounding to nearest even (overflow to Inf is the format's, not an error)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x64, dtype=np.float64).astype(np.float16)


# ------------------------------------------------------------------------------------------------ SiLU * up
def silu64(g16):
    """g / (1 + e^-g) in float64 (e^-g overflows to Inf from g < -709: the quotient is -0, the limit's fp16 value)"""
    g = np.asarray(g16, dtype=np.float16).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return g / (1.0 + np.exp(-g))


def silu_candidates(g16, delta):
    """fp16 [3, n]: fp16(q (1 - delta)), fp16(q), fp16(q (1 + delta)); row 1 is the primary candidate"""
    q = silu64(g16)
    return np.stack([to_half(q * f) for f in (1.0 - delta, 1.0, 1.0 + delta)])


def pair_candidates(g16, u16, delta):
    """fp16 [3, n]: fp16(float64(c) * float64(u)) for each SiLU candidate c of g"""
    u = np.asarray(u16, dtype=np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([to_half(c.astype(np.float64) * u) for c in silu_candidates(g16, delta)])


def same(a16, b16, zero_signs=True):
    """element-wise: the same fp16 value -- NaN by class, everything else by its bits (zero_signs=False: +0 and -0 are one value)"""
    a, b = np.asarray(a16, dtype=np.float16), np.asarray(b16, dtype=np.float16)
    eq = bits(a).reshape(a.shape) == bits(b).reshape(b.shape)
    if not zero_signs:
        eq = eq | ((a == 0) & (b == 0))
    return eq | (np.isnan(a) & np.isnan(b))


def in_candidates(out16, cand, zero_signs=True):
    """(ok, nonprimary): out is one of the candidates [3, n]; it is one, but not the primary one"""
    hit = np.stack([same(out16, c, zero_signs) for c in cand])
    return hit.any(axis=0), hit.any(axis=0) & ~hit[1]


def scramble(i, c):
    """bit pattern i -> another, a bijection of the 16-bit patterns for every row c: an odd multiplier plus an offset, mod 2^16.  Two rows
    c != c' (mod 2^16) send every i to different patterns: the images differ by (c - c')(2 i + 0x3C6F), an odd multiple of c - c'."""
    i = np.asarray(i, dtype=np.int64)
    return ((i * (0x9E37 + 2 * int(c)) + 0x3C6F * (int(c) + 1)) & 0xFFFF).astype(np.uint16)


def scramble_finite(i, c):
    """scramble restricted to the finite patterns (walk the cycle until it is back among them: the induced bijection of FINITE)"""
    out = scramble(i, c)
    for _ in range(64):
        bad = (out & 0x7C00) == 0x7C00
        if not bad.any():
            return out
        out[bad] = scramble(out[bad], c)
    raise AssertionError("a cycle of 64 non-finite patterns")


# ------------------------------------------------------------------------------------------------ the fp8 write
def fp8_codes(x16, inv):
    """kv8_model.quantize on numpy fp16 (any shape) with one fp32 reciprocal scale (or an array broadcast against x16) -> uint8"""
    x = torch.from_numpy(np.ascontiguousarray(x16, dtype=np.float16).copy())
    return k8.quantize(x, torch.as_tensor(inv, dtype=torch.float32)).numpy()


def fp8_ok(codes, want, x16):
    """element-wise: the byte a kernel stored for x16 is right -- equal to the model's `want` for a finite or infinite x16, either NaN code
    for a NaN"""
    codes, want = np.asarray(codes, dtype=np.uint8), np.asarray(want, dtype=np.uint8)
    nan = np.isnan(np.asarray(x16, dtype=np.float16))
    return np.where(nan, (codes & 0x7F) == k8.NAN_CODE, codes == want)


_CODE_VALUES = k8.TABLE.numpy().astype(np.float64)  # code -> value (0x7f / 0xff: NaN)


def fp8_ties(x16, inv):
    """(tie, lower, upper): the inputs whose fp32 product lies exactly halfway between two neighbouring points of the e4m3 grid, and the
    codes of those two points.  The grid is taken with the point 480 that the NaN code 0x7f displaces: at +-464 it is the clamp, not the
    rounding, that decides for 448 -- whose mantissa is the even one as well (`upper` is a NaN code there)."""
    with np.errstate(invalid="ignore"):
        v = np.asarray(x16, dtype=np.float16).astype(np.float32) * np.float32(inv)
    mag = np.abs(v.astype(np.float64))
    grid = np.concatenate([_CODE_VALUES[:0x7F], [480.0]])   # 0 .. 448 ascending with the code, then 480
    lower = np.clip(np.searchsorted(grid, np.where(np.isnan(mag), 0.0, mag), side="right") - 1, 0, 0x7E)
    tie = mag == (grid[lower] + grid[lower + 1]) / 2
    sign = (bits(x16) >> 8).astype(np.uint8) & 0x80
    return tie, lower.astype(np.uint8) | sign, (lower + 1).astype(np.uint8) | sign


# ------------------------------------------------------------------------------------------------ selector layers
def _selector(codes, bits_, first, rows=None):
    from guidedquant_amd import pack
    q = pack.pack_codes(codes, bits_)
    if rows is not None:   # (every row holds the codes of the one given)
        q = np.ascontiguousarray(np.repeat(q, rows, axis=1))
    lut = np.zeros((q.shape[1], 1 << bits_), dtype=np.float16)
    lut[:, 0] = first
    return q, lut


def pair_selector(values16, K, bits_):
    """(qweight, lut, x): N = len(values) rows with code 0 in column 0 and code 1 elsewhere, lut[r] = [v_r, 0, ...], x one-hot at 0.
    y[r] = v_r * 1 + zeros: the planted value, -0 as +0."""
    values16 = np.asarray(values16, dtype=np.float16)
    codes = np.ones((1, K), dtype=np.uint8)
    codes[:, 0] = 0
    x = np.zeros(K, dtype=np.float16)
    x[0] = 1
    return _selector(codes, bits_, values16, rows=values16.size) + (x, )


def prologue_selector(K, bits_):
    """(qweight, lut): N = K rows, row r with code 0 in column r only, lut[r] = [1, 0, ...]: y = the activation vector itself"""
    codes = np.ones((K, K), dtype=np.uint8)
    codes[np.arange(K), np.arange(K)] = 0
    return _selector(codes, bits_, 1.0)


def prologue_ups(g16):
    """u = 2^-e, e = max(exponent of fp16(silu(g)), -15) (e = -15 for a zero): u * fp16(silu(g)) is a multiple of 2^-10 below 2, and u * c
    for every candidate c of g a multiple of 2^-11 of at most 2 (a candidate may lie one ulp away in the binade below or be the power
    of two above).  Any sum of at most 4096 of them is at most 2^24 units of 2^-11: exact in fp32, in any order, like every
    difference of two such sums."""
    s = np.abs(silu_candidates(g16, 0.0)[1].astype(np.float64))
    assert np.isfinite(s).all()
    with np.errstate(divide="ignore"):
        e = np.maximum(np.floor(np.log2(s)), -15.0)   # (log2(0) = -inf -> -15)
    u = (2.0**-e).astype(np.float16)
    assert (u.astype(np.float64) == 2.0**-e).all()
    return u


# ------------------------------------------------------------------------------------------------ injected faults
def faulty_silu(fault, g16, u16):
    """a SiLU * up output with one deviation from the contract (the primary candidate everywhere else)"""
    g16, u16 = np.asarray(g16, dtype=np.float16), np.asarray(u16, dtype=np.float16)
    u, q = u16.astype(np.float64), silu64(g16)
    s = to_half(q)
    if fault == "subnormal_flush":
        s = np.where(np.abs(s) < 2.0**-14, np.copysign(np.float16(0), s), s)
    elif fault == "exp_2^-12":
        g = g16.astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            s = to_half(g / (1.0 + np.exp(-g) * (1.0 + 2.0**-12)))
    elif fault == "neighbours_up":
        u = np.roll(u, -1)
    elif fault == "no_fp16_silu":
        with np.errstate(invalid="ignore"):
            return to_half(q * u)
    else:
        raise AssertionError(fault)
    with np.errstate(invalid="ignore"):
        return to_half(s.astype(np.float64) * u)


def faulty_fp8(fault, x16, inv):
    """the codes of x16 with one deviation from the write rule"""
    x16 = np.asarray(x16, dtype=np.float16)
    codes = fp8_codes(x16, inv)
    with np.errstate(invalid="ignore"):
        v = x16.astype(np.float32) * np.float32(inv)
    sign = (bits(x16) >> 8).astype(np.uint8) & 0x80
    if fault == "truncate":
        pos = _CODE_VALUES[:0x7F]   # 0 .. 448, ascending with the code
        with np.errstate(invalid="ignore"):
            mag = np.clip(np.abs(v.astype(np.float64)), 0.0, 448.0)
        idx = np.searchsorted(pos, np.where(np.isnan(mag), 0.0, mag), side="right") - 1
        return np.where(np.isnan(v), codes, idx.astype(np.uint8) | sign)
    if fault == "ties_away":
        tie, lower, upper = fp8_ties(x16, inv)
        return np.where(tie & ((upper & 0x7F) != k8.NAN_CODE), np.where(codes == lower, upper, lower), codes)
    if fault == "nan_beyond_448":
        with np.errstate(invalid="ignore"):
            return np.where(np.abs(v) > 448.0, np.uint8(k8.NAN_CODE) | sign, codes)
    if fault == "subnormal_codes_flushed":
        return np.where((codes & 0x78) == 0, codes & 0x80, codes)
    if fault == "nan_as_-448":
        return np.where(np.isnan(v), np.uint8(0xFE), codes)
    raise AssertionError(fault)
