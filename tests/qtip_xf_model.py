"""Host model of the QTIP transform side (csrc/fwht.h, csrc/qtip_xform.h, csrc/qtip_xf.hip, the prologue of the fused linear in
csrc/qtip.hip): what every entry point must leave in memory, BIT FOR BIT, in numpy float32 / float16.  No GPU, no library.  Like
tests/halfsweep_model.py and tests/sampler_lp_model.py it restates the CONTRACT -- the order of the additions and the rounding points --
not the kernels: no LDS, no lanes, no passes appear here, only the order they promise ("the arithmetic of a plain radix-2 loop").
The build uses -ffp-contract=off, the factor entries are +-1 and an fp16 square is exact in fp32: no fused multiply-add question arises.

Every rounding point once, with the line it mirrors:
  fwht32(v, P)       fwht.h:10-12     float32; stages h = 1, 2, 4, .. < P with (a + b, a - b) at (j, j + h), over the n / P consecutive
                                      segments of v
  sum_parts          qtip_xform.h:41  float32 adds of the split-K parts, part 0 first
  inv_sqrt(n)        qtip_xf.hip      float32(float64(n) ** -0.5)  (gq_inv_sqrt_f)
  xf_out             qtip_xform.h:57  fp32 v * M^-1/2, fp32 * SV32, then fp16; qtip_xform.h:60: the residual is ONE fp16 add, residual + y
  xf_in              qtip_xform.h:63  NONE / PRE: float(x) * SU.  RMSNORM: half(float(x) * rs) * half(normw) (an fp16 product), then * SU
  rms_scale          qtip_xform.h:107 block_rms_scale: per-thread sums of squares from 0.f in the thread's own order -- "elements":
                                      tid, tid + T, .. (qtip_transform_kernel); "units": the 8 elements of unit tid, then of unit
                                      tid + T, .. (qtip_out_in_kernel, the fused linear's prologue) --, the balanced tree over the 64
                                      lanes by lane bits 0 .. 5 (wave_util.h: wave_allsum), the same tree over the wave sums padded with
                                      zeros to 64, then 1 / sqrt(t / K + eps): a float32 division, add, square root and division
  xf_in_h16          qtip_xform.h:91  fp32 f * K^-1/2, fp32 / 32, then fp16
  factor_product     qtip_xf.hip: qtip_transform_kernel.  KQ = 1024 / P for P < 1024, else 1; kper = ceil(Kf / KQ); group kq sums
                                      its k range [kq kper, min((kq + 1) kper, Kf)) from 0.f in ascending k; the KQ partial sums are
                                      added from 0.f in ascending kq; `transpose` selects hadK[k][r] instead of hadK[r][k].  The scale
                                      comes behind the product.  Nothing depends on the rows per block (RB)
  seg_combine        qtip_xform.h:120 gq_qtip_linear_out_seg: T = 512 threads, Q = 32 units per segment, G = 16 thread groups; thread
                                      tid adds its (up to four) 16-byte units tid + 512 k from 0.f with the sign (-1)^popcount(c & seg),
                                      c = unit / Q; the G partial sums of an element are added from 0.f in ascending order; then the
                                      128-point transform and xf_out with M^-1/2
  prologue_threads   qtip.hip         block size of gq_qtip_linear_in at ksplit 1: 64 * clamp(pow2ceil(ceil(K / 32 / chunk)), 4, 16),
                                      chunk = 4 tile blocks at R = 2, else 2 -- the RMSNorm statistic's tree depends on it
Entry points, built from those: hadamard (gq_hadamard), linear_out, linear_out_seg, linear_out_in, linear_in_xt (the fp16 vector the
fused linear's prologue builds = what a pre-transformed launch takes), factor_transform (gq_qtip_transform), mlp_mid.

SiLU * up (__expf: not reproducible bit for bit).  halfsweep_model.pair_candidates(g, u, DELTA_DECODE) gives per element the fp16
candidates; the value in front of the transform lies between the smallest and the largest, row 1 is the primary.  silumul_in returns the
primary fp32 vector with `lo`, `hi`; silumul_bound(lo, hi, d, scale) = (sum_i (hi_i - lo_i) + 2 d 2^-24 sum_i max(|lo_i|, |hi_i|)) * scale
bounds |out - primary| of every output of a +-1 transform over those elements behind `scale` (d: additions on one output's path;
twice, for the device's and the primary's own rounding), before the output format's own ulp (`ulp16`, `ulp32`).  gq_qtip_transform's
output carries scale = n^-1/2 / 32; z32 of gq_qtip_mlp_mid is the unscaled factor product of one column: scale = 1, the sums over that
column's Kf elements, d = kper + KQ.

d, the additions on one output's path (`depth`): log2 P; + kper + KQ for a factor width; + 4 + 16 for the segmented form.
float64 yardsticks: fwht64, sylvester(n) = (-1)^popcount(i & j), had64 (float64 radix-2 loop, then hadK @).

`fault=` injects ONE deviation (FAULTS), for tests/test_qtip_xf_model_cpu.py only.
"""
import functools

import numpy as np

F32 = np.float32
FAULTS = ("stage_swapped", "last_of_two_skipped", "factor_transposed", "scale_before_product", "parts_descending", "no_half_rs",
          "kq_running_sum")
SWAPPED_STRIDE = 4
HAD_FACTORS = (12, 20, 28, 36, 52, 60, 108, 116, 124, 140, 156, 172)
EPS = 1e-5


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def log2i(n):
    n = int(n)
    assert n > 0 and n & (n - 1) == 0, n
    return n.bit_length() - 1


def inv_sqrt(n):
    return F32(float(n) ** -0.5)


@functools.lru_cache(maxsize=None)
def hadK(Kf):
    """the packaged +-1 factor table of order Kf as float32 [Kf, Kf] (guidedquant_amd/data/hadamard_factors.npz, read as qtip.py does)"""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "guidedquant_amd", "data", "hadamard_factors.npz")
    with np.load(path) as z:
        bits = np.unpackbits(z[f"had{Kf}"])[:Kf * Kf].reshape(Kf, Kf)
    return (bits.astype(np.int8) * 2 - 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the butterflies
def rest_radices(P):
    """the radices of fwht.h's passes behind the first one (fwht_rest), for the fault that needs to know where two stages remain"""
    h0 = 1 if P < 64 else 16 * (32 if P >= 512 else P // 16)
    out = []
    while h0 < P:
        left = P // h0
        rad = 8 if left >= 8 else left
        out.append(rad)
        h0 *= rad
    return out


def fwht32(v, P, fault=None):
    """fwht.h:10-12: stages h = 1, 2, 4, .. with (a + b, a - b) at (j, j + h), float32, over the len(v) / P segments of v"""
    v = _f32(v).reshape(-1).copy()
    P = int(P)
    assert v.size % P == 0
    skip_last = fault == "last_of_two_skipped" and rest_radices(P)[-1:] == [4]
    h = 1
    while h < P:
        if skip_last and 2 * h == P:
            break
        w = v.reshape(-1, 2, h)
        a, b = w[:, 0, :].copy(), w[:, 1, :].copy()
        if fault == "stage_swapped" and h == SWAPPED_STRIDE:
            a, b = b, a
        w[:, 0, :] = a + b
        w[:, 1, :] = a - b
        h *= 2
    return v


def fwht64(v, P):
    v = np.asarray(v, dtype=np.float64).reshape(-1).copy()
    h = 1
    while h < P:
        w = v.reshape(-1, 2, h)
        a, b = w[:, 0, :].copy(), w[:, 1, :].copy()
        w[:, 0, :], w[:, 1, :] = a + b, a - b
        h *= 2
    return v


def sylvester(n):
    i = np.arange(n, dtype=np.int64)
    x = i[:, None] & i[None, :]
    par = np.zeros_like(x)
    while x.any():
        par ^= x & 1
        x >>= 1
    return (1 - 2 * par).astype(np.float64)


def had64(x, hk, P, transpose=False):
    """float64: the P-point transform of every row of the [Kf][P] view, then hadK @ (hadK^T @) over the rows; hk None: P = n"""
    v = fwht64(x, P)
    if hk is None:
        return v
    H = np.asarray(hk, dtype=np.float64)
    return ((H.T if transpose else H) @ v.reshape(H.shape[0], P)).reshape(-1)


def hadamard(x, n, scale, fault=None):
    """gq_hadamard: y = (x @ H_n) * scale, row by row: the butterflies, then one fp32 product"""
    return (fwht32(x, n, fault) * F32(scale)).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------------ element-wise arithmetic
def sum_parts(y32, M, fault=None):
    """qtip_xform.h:41: y32 [parts][M] added in ascending order, part 0 first"""
    y = _f32(y32).reshape(-1, M)
    if fault == "parts_descending":
        y = y[::-1]
    t = y[0].copy()
    for p in range(1, y.shape[0]):
        t = t + y[p]
    return t


def xf_out(v, n, sv32, resid=None):
    """qtip_xform.h:57-61"""
    y = ((_f32(v) * inv_sqrt(n)) * _f32(sv32)).astype(np.float16)
    if resid is not None:
        y = np.asarray(resid, dtype=np.float16) + y
    return y


def _tree64(w):
    """wave_util.h: wave_allsum over the last axis (64 lanes): partners by lane bits 0 .. 5; every lane ends with the same sum"""
    lanes = np.arange(64)
    for b in range(6):
        w = w + w[..., lanes ^ (1 << b)]
    return w[..., 0]


def rms_scale(x16, T, order, eps=EPS):
    """qtip_xform.h:107-118 with the per-thread sums in front of it"""
    x = np.asarray(x16, dtype=np.float16).astype(np.float32).reshape(-1)
    K, T = x.size, int(T)
    sq = x * x
    if order == "elements":
        steps = -(-K // T)
        per = np.zeros(steps * T, dtype=np.float32)
        per[:K] = sq
        per = per.reshape(steps, T)
    else:
        assert order == "units" and K % 8 == 0
        trips = -(-(K // 8) // T)
        per = np.zeros((trips * T, 8), dtype=np.float32)
        per[:K // 8] = sq.reshape(-1, 8)
        per = per.reshape(trips, T, 8).transpose(0, 2, 1).reshape(trips * 8, T)
    ss = np.zeros(T, dtype=np.float32)
    for row in per:
        ss = ss + row
    waves = _tree64(ss.reshape(T // 64, 64))
    pad = np.zeros(64, dtype=np.float32)
    pad[:T // 64] = waves
    t = _tree64(pad)
    return F32(1.0) / np.sqrt(t / F32(K) + F32(eps), dtype=np.float32)


def xf_in(x16, su, rs=None, normw=None, fault=None):
    """qtip_xform.h:63-76 without the SiLU arm (silumul_in): rs None is NONE / PRE"""
    xh = np.asarray(x16, dtype=np.float16)
    if rs is not None:
        t = xh.astype(np.float32) * F32(rs)
        nw = np.asarray(normw, dtype=np.float16)
        if fault == "no_half_rs":
            xh = (t * nw.astype(np.float32)).astype(np.float16)
        else:
            xh = t.astype(np.float16) * nw
    return xh.astype(np.float32) * _f32(su)


def xf_in_h16(f, n):
    """qtip_xform.h:91"""
    return ((_f32(f) * inv_sqrt(n)) / F32(32.0)).astype(np.float16)


def ulp16(a):
    """one fp16 ulp at |a| (the subnormal spacing below 2^-14)"""
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0**-14)))
    return 2.0**(e - 10)


def ulp32(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0**-126)))
    return 2.0**(e - 23)


# ------------------------------------------------------------------------------------------------ power-of-two widths
def linear_out(y32, sv32, resid, M, fault=None):
    """gq_qtip_linear_out (both arms), the transform-out inside gq_qtip_linear_out_in / gq_qtip_linear / the folded prologue"""
    return xf_out(fwht32(sum_parts(y32, M, fault), M, fault), M, sv32, resid)


def seg_combine(y, M):
    """qtip_xform.h:120-151 + qtip_xf.hip: the [M / 128][128] inputs of the 128-point transforms"""
    T, Q, G = 512, 32, 16
    S = M // 128
    units = np.zeros((4 * T, 4), dtype=np.float32)
    units[:M // 4] = _f32(y).reshape(-1, 4)
    units = units.reshape(4, T, 4)
    c = (np.arange(4 * T) // Q).reshape(4, T)
    seg = np.arange(S)
    x = c[None] & seg[:, None, None]
    par = np.zeros_like(x)
    while x.any():
        par ^= x & 1
        x >>= 1
    sg = (1 - 2 * par).astype(np.float32)  # [S, 4, T]
    acc = np.zeros((S, T, 4), dtype=np.float32)
    for k in range(4):
        acc = acc + sg[:, k, :, None] * units[k][None]
    ps = acc.reshape(S, G, Q * 4)
    z = np.zeros((S, Q * 4), dtype=np.float32)
    for gi in range(G):
        z = z + ps[:, gi]
    return z


def linear_out_seg(y32, sv32, resid, M, fault=None):
    z = seg_combine(sum_parts(y32, M, fault), M)
    return xf_out(fwht32(z, 128, fault), M, sv32, resid)


def linear_in_xt(x16, su, rs=None, normw=None, fault=None):
    """the transform-in of a power-of-two width: xf_in, K-point transform, xf_in_h16"""
    K = np.asarray(x16).size
    return xf_in_h16(fwht32(xf_in(x16, su, rs, normw, fault), K, fault), K)


def prologue_threads(K, R=2):
    nch = -(-(K // 32) // (4 if R == 2 else 2))
    w = 1
    while w < 16 and w < nch:
        w *= 2
    return 64 * max(w, 4)


def linear_out_in(y32, sv32, resid, normw, sus, K, eps=EPS, fault=None):
    """gq_qtip_linear_out_in: (hidden, [xt_j]); the statistic in 1024 threads' unit order"""
    hidden = linear_out(y32, sv32, resid, K, fault)
    rs = rms_scale(hidden, 1024, "units", eps)
    return hidden, [linear_in_xt(hidden, su, rs, normw, fault) for su in sus]


# ------------------------------------------------------------------------------------------------ widths with a Hadamard factor
def factor_kq(P):
    return 1024 // P if P < 1024 else 1


def depth(P, Kf=None, seg=False):
    d = log2i(P)
    if Kf:
        KQ = factor_kq(P)
        d += -(-Kf // KQ) + KQ
    return d + (4 + 16 if seg else 0)


def factor_product(V, hk, transpose, fault=None):
    """qtip_transform_kernel's product over the rows of V [Kf][P]: out[r] = sum_k H[r][k] V[k], H = hk or (transpose) hk^T"""
    hk = _f32(hk)
    Kf, P = V.shape
    H = hk.T if bool(transpose) != (fault == "factor_transposed") else hk
    KQ = factor_kq(P)
    kper = -(-Kf // KQ)
    out = np.zeros((Kf, P), dtype=np.float32)
    run = fault == "kq_running_sum"
    for kq in range(KQ):
        acc = out if run else np.zeros((Kf, P), dtype=np.float32)
        for k in range(kq * kper, min((kq + 1) * kper, Kf)):
            acc = acc + H[:, k, None] * V[k][None, :]
        out = acc if run else out + acc
    return out


def _factor(v, hk, P, transpose, n, fault):
    if fault == "scale_before_product":
        return factor_product((fwht32(v, P, fault) * inv_sqrt(n)).reshape(-1, P), hk, transpose, fault).reshape(-1), F32(1.0)
    return factor_product(fwht32(v, P, fault).reshape(-1, P), hk, transpose, fault).reshape(-1), inv_sqrt(n)


def factor_transform_out(y32, sv32, resid, hk, transpose, fault=None):
    """gq_qtip_transform, output side (one part: the entry point takes the sums as they are)"""
    n, Kf = _f32(y32).size, np.shape(hk)[0]
    acc, sc = _factor(y32, hk, n // Kf, transpose, n, fault)
    y = ((acc * sc) * _f32(sv32)).astype(np.float16)
    return y if resid is None else np.asarray(resid, dtype=np.float16) + y


def factor_transform_in(x16, su, hk, transpose, normw=None, eps=EPS, fault=None):
    """gq_qtip_transform, input side, NONE (normw None) or RMSNORM (the statistic in 1024 threads' element order)"""
    n, Kf = np.asarray(x16).size, np.shape(hk)[0]
    rs = None if normw is None else rms_scale(x16, 1024, "elements", eps)
    acc, sc = _factor(xf_in(x16, su, rs, normw, fault), hk, n // Kf, transpose, n, fault)
    return ((acc * sc) / F32(32.0)).astype(np.float16)


# ------------------------------------------------------------------------------------------------ SiLU * up: bounded, not exact
def silumul_in(g16, u16, su):
    """(primary, lo, hi) fp32: xf_in<SILUMUL> for the primary candidate, and the range the device's value lies in"""
    import halfsweep_model as hs
    cand = hs.pair_candidates(g16, u16, hs.DELTA_DECODE).astype(np.float32) * _f32(su)[None]
    return cand[1], cand.min(axis=0), cand.max(axis=0)


def silumul_share(g16, u16):
    """share of the elements with more than one candidate (the condition of the bound: at most 1/16)"""
    import halfsweep_model as hs
    cand = hs.pair_candidates(g16, u16, hs.DELTA_DECODE)
    return float(((hs.bits(cand[0]) != hs.bits(cand[1])) | (hs.bits(cand[2]) != hs.bits(cand[1]))).mean())


def silumul_bound(lo, hi, d, scale):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return ((hi - lo).sum(axis=-1) + 2.0 * d * 2.0**-24 * np.maximum(np.abs(lo), np.abs(hi)).sum(axis=-1)) * scale


def factor_transform_silumul(g16, u16, su, hk, transpose):
    """gq_qtip_transform, input side, SILUMUL: (primary fp16 output, bound on |out - primary| in front of the fp16 ulp)"""
    n, Kf = np.asarray(g16).size, np.shape(hk)[0]
    P = n // Kf
    pri, lo, hi = silumul_in(g16, u16, su)
    acc, sc = _factor(pri, hk, P, transpose, n, None)
    return ((acc * sc) / F32(32.0)).astype(np.float16), silumul_bound(lo, hi, depth(P, Kf), float(n) ** -0.5 / 32.0)


def mlp_mid(y32g, y32u, sv32g, sv32u, su_down, hk):
    """gq_qtip_mlp_mid at n = Kf * 64: (gate_out, up_out) bit for bit = factor_transform_out without a residual, hadK @; z32 [n]: the
    primary of the in product (hadK^T @) of every column, and its bound per column [64] in front of the fp32 ulp"""
    Kf, P = np.shape(hk)[0], 64
    n = Kf * P
    g = factor_transform_out(sum_parts(y32g, n), sv32g, None, hk, 0)
    u = factor_transform_out(sum_parts(y32u, n), sv32u, None, hk, 0)
    pri, lo, hi = silumul_in(g, u, su_down)
    z = factor_product(pri.reshape(Kf, P), hk, 1).reshape(-1)
    d = -(-Kf // 16) + 16
    return g, u, z, silumul_bound(lo.reshape(Kf, P).T, hi.reshape(Kf, P).T, d, 1.0)


# ------------------------------------------------------------------------------------------------ shapes and inputs of the GPU test
# (tests/test_qtip_xf_exact_gpu.py runs them on the device, tests/test_qtip_xf_model_cpu.py checks the model at the same ones)
HADAMARD_N = tuple(1 << i for i in range(16))            # 1 .. 32768
LINEAR_OUT_M = tuple(1 << i for i in range(5, 16))       # 32 .. 32768
SEG_M = tuple(1 << i for i in range(7, 14))              # 128 .. 8192
OUT_IN_K = tuple(1 << i for i in range(8, 14))           # 256 .. 8192
PROLOGUE_K = tuple(1 << i for i in range(7, 15))         # 128 .. 16384
FACTOR_SHAPES = tuple((Kf, 64) for Kf in HAD_FACTORS) + tuple((Kf, P) for P in (128, 256, 512, 1024) for Kf in (12, 20, 28)) + (
    (12, 2048), (108, 128), (108, 256))                  # with 13824 = 108 * 128, 5120 = 20 * 256, 27648 = 108 * 256, 28672 = 28 * 1024
MID_KF = (12, 28, 108, 172)                              # z32 of gq_qtip_mlp_mid; gate_out / up_out: every table
SPIKE = 1024.0                                           # four elements of every vector: 2^10 times the typical magnitude


def case_rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(" ".join(map(str, key)).encode()))


def _spiked(rng, a):
    idx = rng.choice(a.size, min(4, a.size), replace=False)
    a[idx] *= SPIKE
    return a


def in_f16(rng, n):
    """activations ~ N(0, 1) as fp16, four of them * 2^10"""
    return _spiked(rng, rng.standard_normal(n)).astype(np.float16)


def in_sums(rng, parts, n):
    """split-K sums ~ N(0, 1) / 32 as fp32 [parts * n], four of them * 2^10"""
    return _spiked(rng, rng.standard_normal(parts * n) / 32.0).astype(np.float32)


def in_signs(rng, n, mag=1.0):
    return ((rng.integers(0, 2, n) * 2 - 1) * mag).astype(np.float32)


def in_normw(rng, n):
    return (1.0 + 0.2 * rng.standard_normal(n)).astype(np.float16)


def in_gate_up(n):
    """SiLU * up inputs: N(0, 1) gate and up with seed n, four of each * 2^10 at eight different places (a product of two enlarged
    elements would leave the fp16 range)"""
    rng = np.random.default_rng(n)
    g, u = rng.standard_normal(n), rng.standard_normal(n)
    idx = rng.choice(n, 8, replace=False)
    g[idx[:4]] *= SPIKE
    u[idx[4:]] *= SPIKE
    return g.astype(np.float16), u.astype(np.float16)


def in_mlp_mid(Kf, parts):
    """(y32_gate, y32_up, SV32_gate, SV32_up, SU_down) of one gq_qtip_mlp_mid case, n = Kf * 64"""
    n, rng = Kf * 64, case_rng("mlp_mid", Kf, parts)
    return in_sums(rng, parts, n), in_sums(rng, parts, n), in_signs(rng, n, 32.0), in_signs(rng, n, 32.0), in_signs(rng, n)
