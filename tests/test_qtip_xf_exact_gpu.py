"""The QTIP transform side on the device against the exact host model (tests/qtip_xf_model.py), at every length and factor table its
entry points accept: gq_hadamard, gq_qtip_linear_out / _out_seg / _out_in, gq_qtip_transform, gq_qtip_mlp_mid and the prologue of the
fused linear (gq_qtip_linear_in).  Bit for bit, except behind SiLU * up (__expf), where the model's bound holds
(qtip_xf_model.silumul_bound).  The model is tied to float64, to the reference's vectors and to the recorded device digests by
tests/test_qtip_xf_model_cpu.py, which also checks that the model's faults would fail HERE.

Every buffer comes from tests/guarded.py: inputs copied in flush against their guards, outputs left poisoned (an unwritten fp16 element
stays a NaN, an fp32 one 8.4e37), Guards.check() behind every launch.  Inputs are N(0, 1) with four elements of every vector enlarged
2^10 times (qtip_xf_model.in_*), so that a mis-paired element shows at every magnitude.  Launches of one or a few blocks: seconds."""
import ctypes
import os

import numpy as np
import pytest

import qtip_xf_model as m
from guarded import Guards

pytestmark = pytest.mark.gpu
EPS = m.EPS
PRO_NONE, PRO_RMSNORM, PRO_SILUMUL, PRO_PRE = 0, 1, 2, 3


def _api():
    from guidedquant_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream_ptr()


def _off(g, name, a, elems):
    """input `a` placed `elems` elements behind a 16-byte aligned address (the kernels' unaligned arms); the elements in front are
    the guard pattern.  Returns the address of a[0]"""
    a = np.ascontiguousarray(a).reshape(-1)
    pad = np.full(elems * a.itemsize, 0x7E, dtype=np.uint8).view(a.dtype)
    return g.inp(name, np.concatenate([pad, a])).ptr() + elems * a.itemsize


def _same(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.size == want.size, what
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = np.nonzero(got.view(u) != want.view(u))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: device {got[bad[0]]!r}, model {want[bad[0]]!r}"


def _ptr(b):
    return None if b is None else b.ptr()


# ------------------------------------------------------------------------------------------------ gq_hadamard
def _hadamard(x, n, scale):
    _lib, L, st = _api()
    g = Guards()
    xi, yo = g.inp("x", x), g.out("y", x.size * 4)
    _lib.check(L.gq_hadamard(xi.ptr(), yo.ptr(), x.size // n, n, scale, st), "gq_hadamard")
    g.check()
    return yo.numpy(np.float32)


@pytest.mark.parametrize("n", m.HADAMARD_N)
def test_hadamard_every_length(n):
    for rows in (1, 3):
        x = m.in_sums(m.case_rng("hadamard", n, rows), rows, n)
        for scale in (float(m.inv_sqrt(n)), 1.0):
            _same(_hadamard(x, n, scale), m.hadamard(x, n, scale), f"gq_hadamard n {n} rows {rows} scale {scale}")
    if n <= 2048:
        got = _hadamard(np.eye(n, dtype=np.float32), n, 1.0)
        assert (got.reshape(n, n) == m.sylvester(n)).all(), f"gq_hadamard of the identity is not the Sylvester matrix, n {n}"


# ------------------------------------------------------------------------------------------------ gq_qtip_linear_out / _out_seg
def _out_inputs(key, Ms, parts, resid):
    rng = m.case_rng(*key)
    return [(m.in_sums(rng, parts, M), m.in_signs(rng, M, 32.0), m.in_f16(rng, M) if resid else None) for M in Ms]


def _linear_out(entry, Ms, ins, parts, y_off=0):
    _lib, L, st = _api()
    g = Guards()
    descs, outs = [], []
    for i, (M, (y, sv, res)) in enumerate(zip(Ms, ins)):
        yp = _off(g, f"y32_{i}", y, y_off) if y_off else g.inp(f"y32_{i}", y).ptr()
        o = g.out(f"out{i}", M * 2)
        outs.append(o)
        descs.append(_lib.GqQtipOut(yp, g.inp(f"sv{i}", sv).ptr(), _ptr(g.inp(f"resid{i}", res)), o.ptr(), M, parts))
    _lib.check(getattr(L, entry)(len(Ms), (_lib.GqQtipOut * len(Ms))(*descs), st), entry)
    g.check()
    return [o.numpy(np.float16) for o in outs]


@pytest.mark.parametrize("M", m.LINEAR_OUT_M)
def test_linear_out_every_length_both_arms(M):
    """the vector arm (everything aligned, M <= 8192) and the element arm (the sums 4 bytes off the 16-byte grid; M > 8192 has no other)"""
    for parts in (1, 4):
        for resid in (0, 1):
            ins = _out_inputs(("linear_out", M, parts, resid), [M], parts, resid)
            want = m.linear_out(*ins[0], M)
            for y_off in (0, 1):
                got = _linear_out("gq_qtip_linear_out", [M], ins, parts, y_off)[0]
                _same(got, want, f"gq_qtip_linear_out M {M} parts {parts} resid {resid} sums +{4 * y_off} B")


def test_linear_out_three_linears_of_different_length():
    Ms = [4096, 32, 512]
    ins = _out_inputs(("linear_out three",), Ms, 4, 1)
    for i, got in enumerate(_linear_out("gq_qtip_linear_out", Ms, ins, 4)):
        _same(got, m.linear_out(*ins[i], Ms[i]), f"gq_qtip_linear_out, linear {i} of {Ms}")


@pytest.mark.parametrize("M", m.SEG_M)
def test_linear_out_seg_every_length(M):
    for parts in (1, 2):
        for resid in (0, 1):
            ins = _out_inputs(("linear_out_seg", M, parts, resid), [M], parts, resid)
            got = _linear_out("gq_qtip_linear_out_seg", [M], ins, parts)[0]
            _same(got, m.linear_out_seg(*ins[0], M), f"gq_qtip_linear_out_seg M {M} parts {parts} resid {resid}")


def test_linear_out_seg_three_linears_short_ones_write_nothing_more():
    """grid = (1024 / 128, 3): the blocks beyond a short linear must write nothing (its guards sit flush behind its 256 / 128 outputs)"""
    Ms = [1024, 256, 128]
    for parts in (1, 2):
        ins = _out_inputs(("linear_out_seg three", parts), Ms, parts, 1)
        for i, got in enumerate(_linear_out("gq_qtip_linear_out_seg", Ms, ins, parts)):
            _same(got, m.linear_out_seg(*ins[i], Ms[i]), f"gq_qtip_linear_out_seg, linear {i} of {Ms}, parts {parts}")


# ------------------------------------------------------------------------------------------------ gq_qtip_linear_out_in
@pytest.mark.parametrize("K", m.OUT_IN_K)
def test_linear_out_in_every_length(K):
    _lib, L, st = _api()
    for parts in (1, 3):
        rng = m.case_rng("linear_out_in", K, parts)
        y, sv, res, nw = m.in_sums(rng, parts, K), m.in_signs(rng, K, 32.0), m.in_f16(rng, K), m.in_normw(rng, K)
        sus = [m.in_signs(rng, K) for _ in range(3)]
        g = Guards()
        h, xt = g.out("hidden", K * 2), [g.out(f"xt{j}", K * 2) for j in range(3)]
        prev = (_lib.GqQtipOut * 1)(_lib.GqQtipOut(g.inp("y32", y).ptr(), g.inp("sv", sv).ptr(), g.inp("resid", res).ptr(), h.ptr(), K, parts))
        sup = (ctypes.c_void_p * 3)(*[g.inp(f"su{j}", s).ptr() for j, s in enumerate(sus)])
        xtp = (ctypes.c_void_p * 3)(*[t.ptr() for t in xt])
        _lib.check(L.gq_qtip_linear_out_in(prev, g.inp("normw", nw).ptr(), EPS, 3, sup, xtp, st), "gq_qtip_linear_out_in")
        g.check()
        wh, wxt = m.linear_out_in(y, sv, res, nw, sus, K)
        _same(h.numpy(np.float16), wh, f"gq_qtip_linear_out_in K {K} parts {parts}: hidden")
        for j in range(3):
            _same(xt[j].numpy(np.float16), wxt[j], f"gq_qtip_linear_out_in K {K} parts {parts}: xt{j}")


# ------------------------------------------------------------------------------------------------ gq_qtip_transform
def _transform_out(Kf, P, transpose, lins):
    """lins: [(y32, sv32, resid)]"""
    _lib, L, st = _api()
    n, g = Kf * P, Guards()
    hk = g.inp("hadK", m.hadK(Kf))
    outs = [g.out(f"out{i}", n * 2) for i in range(len(lins))]
    xf = (_lib.GqQtipXf * len(lins))(*[_lib.GqQtipXf(g.inp(f"y32_{i}", y).ptr(), g.inp(f"sv{i}", sv).ptr(), hk.ptr(), _ptr(g.inp(f"resid{i}", res)),
                                                      outs[i].ptr()) for i, (y, sv, res) in enumerate(lins)])
    _lib.check(L.gq_qtip_transform(0, None, None, None, 0.0, 0, len(lins), xf, n, Kf, transpose, st), "gq_qtip_transform out")
    g.check()
    return [o.numpy(np.float16) for o in outs]


def _transform_in(Kf, P, transpose, pro, x, x2, nw, sus):
    _lib, L, st = _api()
    n, g = Kf * P, Guards()
    hk = g.inp("hadK", m.hadK(Kf))
    outs = [g.out(f"out{i}", n * 2) for i in range(len(sus))]
    xf = (_lib.GqQtipXf * len(sus))(*[_lib.GqQtipXf(None, g.inp(f"su{i}", su).ptr(), hk.ptr(), None, outs[i].ptr()) for i, su in enumerate(sus)])
    _lib.check(L.gq_qtip_transform(1, g.inp("x", x).ptr(), _ptr(g.inp("x2", x2 if pro == PRO_SILUMUL else None)),
                                   _ptr(g.inp("normw", nw if pro == PRO_RMSNORM else None)), EPS, pro, len(sus), xf, n, Kf, transpose, st),
               "gq_qtip_transform in")
    g.check()
    return [o.numpy(np.float16) for o in outs]


def _xf_inputs(Kf, P, n_lin=1):
    n, rng = Kf * P, m.case_rng("transform", Kf, P, n_lin)
    outs = [(m.in_sums(rng, 1, n), m.in_signs(rng, n, 32.0), m.in_f16(rng, n)) for _ in range(n_lin)]
    return outs, m.in_f16(rng, n), m.in_normw(rng, n), [m.in_signs(rng, n) for _ in range(n_lin)]


def _check_transform(Kf, P, what=""):
    hk = m.hadK(Kf)
    outs, x, nw, sus = _xf_inputs(Kf, P)
    for tr in (0, 1):
        _same(_transform_out(Kf, P, tr, outs)[0], m.factor_transform_out(*outs[0], hk, tr), f"gq_qtip_transform out {Kf} x {P} transpose {tr}{what}")
        for pro in (PRO_NONE, PRO_RMSNORM):
            _same(_transform_in(Kf, P, tr, pro, x, None, nw, sus)[0], m.factor_transform_in(x, sus[0], hk, tr, nw if pro else None),
                  f"gq_qtip_transform in prologue {pro} {Kf} x {P} transpose {tr}{what}")


@pytest.mark.parametrize("Kf,P", m.FACTOR_SHAPES)
def test_transform_every_table_and_row_length(Kf, P):
    _check_transform(Kf, P)


def test_transform_two_and_three_linears_in_one_launch():
    for Kf, P, n_lin in ((28, 64, 2), (12, 128, 3), (20, 256, 3)):
        hk = m.hadK(Kf)
        outs, x, nw, sus = _xf_inputs(Kf, P, n_lin)
        for i, got in enumerate(_transform_out(Kf, P, 0, outs)):
            _same(got, m.factor_transform_out(*outs[i], hk, 0), f"gq_qtip_transform out {Kf} x {P}, linear {i} of {n_lin}")
        for i, got in enumerate(_transform_in(Kf, P, 1, PRO_RMSNORM, x, None, nw, sus)):
            _same(got, m.factor_transform_in(x, sus[i], hk, 1, nw), f"gq_qtip_transform in {Kf} x {P}, linear {i} of {n_lin}")


@pytest.fixture
def _rb_env():
    from guidedquant_amd import _lib
    yield
    os.environ.pop("GQ_QTIP_XF_RB", None)
    _lib.lib().gq_reset_env_cache()


@pytest.mark.parametrize("RB", [1, 2, 3, 4])
def test_transform_bits_do_not_depend_on_the_rows_per_block(_rb_env, RB):
    """GQ_QTIP_XF_RB forced: 3 leaves a tail block (28 = 9 * 3 + 1, 20 = 6 * 3 + 2); the host sizes the partial sums [KQ][RB][P] with
    the forced value, the one the kernel indexes them with"""
    from guidedquant_amd import _lib
    os.environ["GQ_QTIP_XF_RB"] = str(RB)
    _lib.lib().gq_reset_env_cache()
    for Kf, P in ((28, 64), (20, 256)):
        _check_transform(Kf, P, f" RB {RB}")


# ------------------------------------------------------------------------------------------------ behind SiLU * up: bounded
def _report(what, err, allowed):
    share = float((err / allowed).max())
    print(f"SILUMUL-SHARE {what}: largest |out - primary| / bound = {share:.4f}")
    return share


@pytest.mark.parametrize("Kf,P", m.FACTOR_SHAPES)
def test_transform_silumul_within_the_candidate_bound(Kf, P):
    n, hk = Kf * P, m.hadK(Kf)
    gate, up = m.in_gate_up(n)
    su = m.in_signs(m.case_rng("silumul", Kf, P), n)
    assert m.silumul_share(gate, up) <= 1 / 16
    for tr in (0, 1):
        got = _transform_in(Kf, P, tr, PRO_SILUMUL, gate, up, None, [su])[0].astype(np.float64)
        pri, bound = m.factor_transform_silumul(gate, up, su, hk, tr)
        pri = pri.astype(np.float64)
        assert np.isfinite(got).all()
        err, allowed = np.abs(got - pri), bound + m.ulp16(np.maximum(np.abs(got), np.abs(pri)))
        _report(f"transform {Kf} x {P} transpose {tr}", err, allowed)
        assert (err <= allowed).all(), (Kf, P, tr, float((err / allowed).max()))


# ------------------------------------------------------------------------------------------------ gq_qtip_mlp_mid
@pytest.mark.parametrize("Kf", m.HAD_FACTORS)
def test_mlp_mid_every_table(Kf):
    """gate_out / up_out bit for bit for every table; z32 within the bound (asserted for every table, Kf = 12, 28, 108, 172 among them)"""
    _lib, L, st = _api()
    n, hk = Kf * 64, m.hadK(Kf)
    for parts in (1, 2):
        yg, yu, svg, svu, sud = m.in_mlp_mid(Kf, parts)
        g = Guards()
        z32, g16, u16 = g.out("z32", n * 4), g.out("gate_out", n * 2), g.out("up_out", n * 2)
        mid = _lib.GqQtipMid(g.inp("y32g", yg).ptr(), g.inp("y32u", yu).ptr(), g.inp("svg", svg).ptr(), g.inp("svu", svu).ptr(),
                             g.inp("hadT16", np.ascontiguousarray(hk.T).astype(np.float16)).ptr(), g.inp("sud", sud).ptr(),
                             g.inp("had16", hk.astype(np.float16)).ptr(), z32.ptr(), g16.ptr(), u16.ptr())
        _lib.check(L.gq_qtip_mlp_mid(ctypes.pointer(mid), parts, n, Kf, st), "gq_qtip_mlp_mid")
        g.check()
        wg, wu, wz, bound = m.mlp_mid(yg, yu, svg, svu, sud, hk)
        _same(g16.numpy(np.float16), wg, f"gq_qtip_mlp_mid Kf {Kf} parts {parts}: gate_out")
        _same(u16.numpy(np.float16), wu, f"gq_qtip_mlp_mid Kf {Kf} parts {parts}: up_out")
        assert m.silumul_share(wg, wu) <= 1 / 16
        got, pri = z32.numpy(np.float32).astype(np.float64).reshape(Kf, 64), wz.astype(np.float64).reshape(Kf, 64)
        assert np.isfinite(got).all()
        err, allowed = np.abs(got - pri), bound[None, :] + m.ulp32(np.maximum(np.abs(got), np.abs(pri)))
        _report(f"mlp_mid z32 Kf {Kf} parts {parts}", err, allowed)
        assert (err <= allowed).all(), (Kf, parts, float((err / allowed).max()))


# ------------------------------------------------------------------------------------------------ the fused linear's prologue
def _linear_in(K, pro, x, nw, su, trellis, tlut, M, R, su_off=0):
    _lib, L, st = _api()
    g = Guards()
    y32 = g.out("y32", M * 4)
    sup = None if su is None else (_off(g, "su", su, su_off) if su_off else g.inp("su", su).ptr())
    arr = (_lib.GqQtipIn * 1)(_lib.GqQtipIn(g.inp("trellis", trellis).ptr(), sup, g.inp("tlut", tlut).ptr(), y32.ptr(), M))
    _lib.check(L.gq_qtip_linear_in(g.inp("x", x).ptr(), None, _ptr(g.inp("normw", nw if pro == PRO_RMSNORM else None)), EPS, pro, K, R, 1, arr,
                                   0, None, 1, st), "gq_qtip_linear_in")
    g.check()
    return y32.numpy(np.float32)


def _check_prologue(K, pro, su_off=0):
    M, R = 64, 2
    rng = m.case_rng("prologue", K, pro)
    x, nw, su = m.in_f16(rng, K), m.in_normw(rng, K), m.in_signs(rng, K)
    trellis = rng.integers(0, 2**32, size=R * M * K // 32, dtype=np.uint32)
    tlut = (0.02 * rng.standard_normal(1024)).astype(np.float16)
    rs = m.rms_scale(x, m.prologue_threads(K, R), "units", EPS) if pro == PRO_RMSNORM else None
    xt = m.linear_in_xt(x, su, rs, nw)
    fused = _linear_in(K, pro, x, nw, su, trellis, tlut, M, R, su_off)
    pre = _linear_in(K, PRO_PRE, xt, None, None, trellis, tlut, M, R)
    assert np.isfinite(fused).all() and np.isfinite(pre).all()
    _same(fused, pre, f"gq_qtip_linear_in K {K} prologue {pro} SU +{4 * su_off} B against the model's pre-transformed input")


@pytest.mark.parametrize("pro", [PRO_NONE, PRO_RMSNORM])
@pytest.mark.parametrize("K", m.PROLOGUE_K)
def test_fused_linear_prologue_builds_the_models_vector(K, pro):
    """y32 of the launch that transforms x itself == y32 of the same launch handed the MODEL's transform-in vector pre-transformed"""
    _check_prologue(K, pro)


def test_prologue_comparison_sees_one_ulp_of_one_element():
    """the control of the test above: y32 moves when ONE element of the pre-transformed vector moves by one fp16 ulp"""
    K, M, R = 1024, 64, 2
    rng = m.case_rng("prologue control")
    x, su = m.in_f16(rng, K), m.in_signs(rng, K)
    trellis = rng.integers(0, 2**32, size=R * M * K // 32, dtype=np.uint32)
    tlut = (0.02 * rng.standard_normal(1024)).astype(np.float16)
    xt = m.linear_in_xt(x, su)
    off = xt.copy()
    off.view(np.uint16)[K // 3] ^= 1
    a, b = (_linear_in(K, PRO_PRE, v, None, None, trellis, tlut, M, R) for v in (xt, off))
    assert (a.view(np.uint32) != b.view(np.uint32)).sum() >= M // 2


def test_fused_linear_prologue_second_arm():
    """SU 4 bytes off the 16-byte grid: the inputs are read from memory, element by element"""
    _check_prologue(1024, PRO_RMSNORM, su_off=1)
    _check_prologue(16384, PRO_RMSNORM, su_off=1)
