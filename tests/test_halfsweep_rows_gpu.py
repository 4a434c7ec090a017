"""GPU: every fp16 bit pattern through the two per-element rounding points of the prompt pass (csrc/prefill.hip), through the C ABI on
guard-banded buffers (tests/guarded.py), against the host model tests/halfsweep_model.py.

gq_silu_mul_rows         S = 4 rows of 65 536 gates: column i of every row holds bit pattern i (the NaNs, +-Inf, +-0 and the subnormals
                         included), the up of row s is scramble(i, s).  Every output must be one of pair_candidates(.., DELTA_ROWS = 2^-21):
                         NaN by class, zeros with their sign.  Both `paired` orders.
                         Measured on an MI355X: 2 of 262 144 outputs are not the primary candidate, in either order -- both at the
                         gate 2^-24, whose SiLU is a hair above the tie between 0 and 2^-24 (torch's own fp32 SiLU lands there too).
gq_rope_cache_rows_kv8   the fp8 (e4m3) write rule, fp8_quant8.  512 tokens of 2 + 2 + 2 heads of 128: each KV head's v rows carry all 65 536
                         patterns (v is stored as it is), each KV head's k rows the 63 488 finite ones under cos = 1 / sin = 0 tables (the
                         rotation is then the identity up to the sign of zero).  As in tests/test_kv8_rows_gpu.py the expected bytes are
                         kv8_model.quantize of what the fp16 entry wrote for the same inputs: a finite value or an Inf must give the
                         model's byte, a NaN one of the two NaN codes (0x7f / 0xff) -- the rule include/gq_hip.h states.  Scale sets ones /
                         pow2 / free (kv8_model.scale_sets), forms plain / qknorm / bias (a zero bias: v is still the sweep).
                         Found with this test: the clamp (v_med3_f32) returned -448 for a NaN, which was stored as the finite code 0xfe
                         (4 092 bytes of a sweep) -- an fp8 cache hid a NaN activation that an fp16 cache shows as NaN logits.  The kv8
                         instances now store a NaN as a NaN code (0x7f whatever its sign: v_cvt_pk_fp8_f32).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import halfsweep_model as hs  # noqa: E402
import kv8_model as k8  # noqa: E402
from guarded import Guards  # noqa: E402

S_ROWS, INTER = 4, 65536
H, HKV, HD, S, MAX_SEQ = 2, 2, 128, 512, 512
EPS = 1e-6


def _L():
    from guidedquant_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def silu_case():
    """gates, ups [4][65536] (bit patterns) and their candidates at DELTA_ROWS"""
    gate = np.broadcast_to(hs.PATTERNS, (S_ROWS, INTER)).copy()
    up = np.stack([hs.scramble(hs.PATTERNS, s) for s in range(S_ROWS)])
    cand = hs.pair_candidates(hs.half(gate.reshape(-1)), hs.half(up.reshape(-1)), hs.DELTA_ROWS)
    return gate, up, cand


@pytest.mark.parametrize("paired", [0, 1], ids=["halves", "paired"])
def test_silu_mul_rows_over_every_gate(silu_case, paired):
    _lib = _L()
    gate, up, cand = silu_case
    y = np.stack([gate, up], axis=2).reshape(S_ROWS, 2 * INTER) if paired else np.concatenate([gate, up], axis=1)
    g = Guards()
    yb, out = g.inp("y", y), g.out("out", S_ROWS * INTER * 2)
    _lib.check(_lib.lib().gq_silu_mul_rows(yb.ptr(), out.ptr(), S_ROWS, INTER, paired, None), "gq_silu_mul_rows")
    g.check()
    got = out.numpy(np.float16)
    ok, nonprimary = hs.in_candidates(got, cand)
    print(f"gq_silu_mul_rows paired={paired}: {int(nonprimary.sum())} of {ok.size} outputs are not the primary candidate"
          + (f", gates {hs.half(gate.reshape(-1)[nonprimary])[:8]}" if nonprimary.any() else ""))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%d outputs outside their candidates; (gate, up, got, primary) bits: %s" % (
        bad.size, [(hex(gate.reshape(-1)[i]), hex(up.reshape(-1)[i]), hex(hs.bits(got)[i]), hex(hs.bits(cand[1])[i])) for i in bad[:6]])


# ------------------------------------------------------------------------------------------------ the fp8 cache write
@pytest.fixture(scope="module")
def kv8_inputs():
    """qkv [S][(H + 2 Hkv) HD] as bit patterns: q random and small; the k rows of KV head g hold the finite patterns (the 2048 slots left
    over repeat the first ones), scrambled for g = 1; its v rows hold all 65 536 patterns, scrambled likewise.  Token s goes to position
    (197 s + 31) mod 512."""
    rng = np.random.default_rng(5)
    qkv = np.zeros((S, H + 2 * HKV, HD), dtype=np.uint16)
    qkv[:, :H] = hs.bits(rng.normal(0, 1, (S, H, HD)).astype(np.float16)).reshape(S, H, HD)
    fin = np.concatenate([hs.FINITE, hs.FINITE[:S * HD - hs.FINITE.size]])
    for g in range(HKV):
        qkv[:, H + g] = (fin if g == 0 else hs.scramble_finite(fin, g)).reshape(S, HD)
        qkv[:, H + HKV + g] = (hs.PATTERNS if g == 0 else hs.scramble(hs.PATTERNS, g)).reshape(S, HD)
    for g in range(HKV):
        assert np.array_equal(np.unique(qkv[:, H + HKV + g]), hs.PATTERNS) and np.array_equal(np.unique(qkv[:, H + g]), hs.FINITE)
    pos = (197 * np.arange(S) + 31) % MAX_SEQ
    assert np.array_equal(np.sort(pos), np.arange(MAX_SEQ))
    return torch.from_numpy(qkv.reshape(S, -1).view(np.float16).copy()), torch.from_numpy(pos.astype(np.int32))


@pytest.fixture(scope="module")
def fp16_rows(kv8_inputs):
    """form -> (q_out, k cache, v cache) of the fp16 entries on the same inputs, as numpy fp16: the reference of every scale set"""
    _lib = _L()
    L = _lib.lib()
    qkv, pos = kv8_inputs
    one = torch.ones(MAX_SEQ, HD, dtype=torch.float16)
    w = torch.ones(HD, dtype=torch.float16)
    out = {}
    for form in ("plain", "qknorm", "bias"):
        g = Guards()
        rows = (qkv + torch.zeros_like(qkv[0])) if form == "bias" else qkv   # (one fp16 add per element: -0 + 0 = +0)
        b = dict(qkv=g.inp("qkv", rows), pos=g.inp("pos", pos), cos=g.inp("cos", one), sin=g.inp("sin", torch.zeros_like(one)), w=g.inp("w", w))
        q, kc, vc = g.out("q", H * S * HD * 2), g.out("kc", HKV * MAX_SEQ * HD * 2), g.out("vc", HKV * MAX_SEQ * HD * 2)
        if form == "qknorm":
            rc = L.gq_qknorm_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), S, H, HKV, HD,
                                             MAX_SEQ, b["w"].ptr(), b["w"].ptr(), EPS, None)
        else:
            rc = L.gq_rope_cache_rows(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), S, H, HKV, HD, MAX_SEQ, None)
        _lib.check(rc, "fp16 entry")
        g.check()
        out[form] = (q.numpy(np.uint16), kc.numpy(np.float16, (HKV, MAX_SEQ, HD)), vc.numpy(np.float16, (HKV, MAX_SEQ, HD)))
    # the sweep arrives: v as it was sent (every pattern), k up to the sign of zero in the forms without a norm
    qkv_bits = qkv.numpy().view(np.uint16).reshape(S, H + 2 * HKV, HD)
    inv_pos = np.argsort(pos.numpy())
    for form in ("plain", "qknorm"):
        assert np.array_equal(hs.bits(out[form][2]).reshape(HKV, MAX_SEQ, HD), qkv_bits[inv_pos][:, H + HKV:].transpose(1, 0, 2))
    assert hs.same(out["plain"][1], hs.half(qkv_bits[inv_pos][:, H:H + HKV].transpose(1, 0, 2).copy()).reshape(HKV, MAX_SEQ, HD), zero_signs=False).all()
    return out


@pytest.mark.parametrize("scales", ["ones", "pow2", "free"])
@pytest.mark.parametrize("form", ["plain", "qknorm", "bias"])
def test_kv8_write_rule_over_every_pattern(kv8_inputs, fp16_rows, form, scales):
    _lib = _L()
    qkv, pos = kv8_inputs
    q16, k16, v16 = fp16_rows[form]
    ks, vs = k8.scale_sets(HKV)[scales]
    k_inv, v_inv = torch.reciprocal(ks), torch.reciprocal(vs)
    one = torch.ones(MAX_SEQ, HD, dtype=torch.float16)
    g = Guards()
    w = g.inp("w", torch.ones(HD, dtype=torch.float16)) if form == "qknorm" else None
    bias = g.inp("bias", torch.zeros_like(qkv[0])) if form == "bias" else None
    b = dict(qkv=g.inp("qkv", qkv), pos=g.inp("pos", pos), cos=g.inp("cos", one), sin=g.inp("sin", torch.zeros_like(one)), k_inv=g.inp("k_inv", k_inv),
             v_inv=g.inp("v_inv", v_inv))
    q, kc, vc = g.out("q", H * S * HD * 2), g.out("kc", HKV * MAX_SEQ * HD), g.out("vc", HKV * MAX_SEQ * HD)
    opt = lambda x: None if x is None else x.ptr()  # noqa: E731
    rc = _lib.lib().gq_rope_cache_rows_kv8(b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr(), q.ptr(), kc.ptr(), vc.ptr(), b["k_inv"].ptr(),
                                           b["v_inv"].ptr(), S, H, HKV, HD, MAX_SEQ, opt(w), opt(w), EPS, opt(bias), None)
    _lib.check(rc, "gq_rope_cache_rows_kv8")
    g.check()
    assert np.array_equal(q.numpy(np.uint16), q16), "q_out differs from the fp16 entry's"
    for name, got, ref, inv in (("k", kc, k16, k_inv), ("v", vc, v16, v_inv)):
        got = got.numpy(np.uint8, (HKV, MAX_SEQ, HD))
        want = hs.fp8_codes(ref, inv[:, None, None])
        ok = hs.fp8_ok(got, want, ref)
        nan = np.isnan(ref)
        bad = np.argwhere(~ok)
        assert bad.size == 0, "%s cache: %d byte(s) break the write rule (%d of them at a NaN); (fp16 bits, got, want): %s" % (
            name, len(bad), int((~ok & nan).sum()), [(hex(hs.bits(ref).reshape(ref.shape)[tuple(i)]), hex(got[tuple(i)]), hex(want[tuple(i)])) for i in bad[:6]])
        if form == "plain":   # (the case is the whole domain, not a sample of it: every pattern in, every code out -- no NaN code for k)
            assert np.unique(hs.bits(ref)).size >= (65536 if name == "v" else 63487)
            codes = np.unique(got)
            assert np.array_equal(codes[(codes & 0x7F) != k8.NAN_CODE], np.setdiff1d(np.arange(256), [0x7F, 0xFF]))
            assert ((codes & 0x7F) == k8.NAN_CODE).any() == (name == "v")
