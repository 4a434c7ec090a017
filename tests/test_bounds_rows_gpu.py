"""GPU: the prompt pass's row kernels (csrc/prefill.hip) with every buffer guard-banded and poisoned (tests/guarded.py), at their
smallest and raggedest shapes.  Results against the torch expressions tests/test_prefill_native_gpu.py uses (RMSNorm module, F.silu * up,
apply_rotary_pos_emb: RoPE and the cache write bit for bit) and, for the Qwen3 form, the restatement and bound of
tests/test_qknorm_attn_gpu.py (one fp16 spacing at the tensor's largest magnitude; v bit for bit).  Guards: exact equality.

  gq_rmsnorm_rows            D in {8, 520, 2056, 16384} (one 16-byte unit; a partly filled thread pass; more than one pass with a
                             tail; the widest row served), S in {1, 3}, with and without delta
  gq_silu_mul_rows           inter in {8, 1032}, S in {1, 3}, both row orders
  gq_(qknorm_)rope_cache_rows  head_dim in {64, 128} (+ 16, 80 for the plain form), (H, Hkv) in {(1, 1), (5, 1), (6, 2)}, S in {1, 7},
                             positions out of order that include the first and the last cache row and, at S = 7, two positions
                             >= max_seq: their K / V rows are not written anywhere, their q rows are
"""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import guarded  # noqa: E402
from test_prefill_native_gpu import _ulp_close  # noqa: E402
from test_qknorm_attn_gpu import _qknorm, _rope, _spacing  # noqa: E402

MAX_SEQ = 11
FILL = 7.0


def _L():
    from guidedquant_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator(device="cuda:0").manual_seed(seed)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [8, 520, 2056, 16384])
def test_guarded_rmsnorm_rows(S, D):
    from guidedquant_amd.model import RMSNorm
    L = _L()
    d = torch.device("cuda:0")
    g = _gen(S + D)
    x = (torch.randn(S, D, device=d, generator=g) * (torch.rand(S, 1, device=d, generator=g) * 8 + 0.1)).half()
    delta = torch.randn(S, D, device=d, generator=g).half()
    norm = RMSNorm(D, eps=1e-5).to(d).half()
    norm.weight.data.copy_((1 + 0.2 * torch.randn(D, device=d, generator=g)).half())
    for with_delta in (False, True):
        gb = guarded.Guards()
        xb, wb = gb.inp("x", x), gb.inp("weight", norm.weight.data)
        db = gb.inp("delta", delta) if with_delta else None
        ob = gb.out("out", 2 * S * D)
        L.check(L.lib().gq_rmsnorm_rows(xb.ptr(), guarded.ptr(db), wb.ptr(), ob.ptr(), S, D, norm.eps, L.current_stream_ptr()), "gq_rmsnorm_rows")
        gb.check()
        xs = x + delta if with_delta else x
        # x is written back only with delta (x = x + delta, one fp16 add), and is untouched without
        assert torch.equal(xb.view(torch.int16, (S, D)), xs.view(torch.int16))
        _ulp_close(ob.view(torch.float16, (S, D)), norm(xs), ulps=2)


@pytest.mark.parametrize("paired", [0, 1])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("inter", [8, 1032])
def test_guarded_silu_mul_rows(S, inter, paired):
    import torch.nn.functional as F
    L = _L()
    d = torch.device("cuda:0")
    y = (torch.randn(S, 2 * inter, device=d, generator=_gen(S + inter + paired)) * 3).half()
    gate, up = (y[:, 0::2], y[:, 1::2]) if paired else (y[:, :inter], y[:, inter:])
    want = (F.silu(gate) * up).contiguous()
    gb = guarded.Guards()
    yb, ob = gb.inp("y", y), gb.out("out", 2 * S * inter)
    L.check(L.lib().gq_silu_mul_rows(yb.ptr(), ob.ptr(), S, inter, paired, L.current_stream_ptr()), "gq_silu_mul_rows")
    gb.check()
    _ulp_close(ob.view(torch.float16, (S, inter)), want)


def _positions(S):
    """S = 1: the last cache row; S = 7: out of order, the first and the last row among them, two tokens beyond the cache"""
    return [MAX_SEQ - 1] if S == 1 else [4, 0, MAX_SEQ + 3, MAX_SEQ - 1, 2, MAX_SEQ, 7]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("H,Hkv", [(1, 1), (5, 1), (6, 2)])
@pytest.mark.parametrize("hd", [16, 64, 80, 128])
def test_guarded_rope_cache_rows(hd, H, Hkv, S, norm):
    from guidedquant_amd.model import rope_tables
    L = _L()
    d = torch.device("cuda:0")
    if norm and hd not in (64, 128):   # the Qwen3 form serves 64 and 128 only: refused, not launched
        z = guarded.Guarded.empty(64)
        assert L.lib().gq_qknorm_rope_cache_rows(*([z.ptr()] * 7), S, H, Hkv, hd, MAX_SEQ, z.ptr(), z.ptr(), 1e-6, None) == L.GQ_ENOTSUP
        z.check("stand-in")
        return
    g = _gen(hd + 10 * H + S)
    cos, sin = rope_tables(hd, MAX_SEQ, 500000.0, d)
    qkv = torch.randn(S, (H + 2 * Hkv) * hd, device=d, generator=g).half()
    pos = torch.tensor(_positions(S), dtype=torch.int32, device=d)
    qw, kw = ((1 + 0.3 * torch.randn(hd, device=d, generator=g)).half() for _ in range(2))
    gb = guarded.Guards()
    qkvb, posb, cosb, sinb = gb.inp("qkv", qkv), gb.inp("pos", pos), gb.inp("cos", cos), gb.inp("sin", sin)
    kcb = gb.inp("k_cache", torch.full((Hkv, MAX_SEQ, hd), FILL, dtype=torch.float16, device=d))
    vcb = gb.inp("v_cache", torch.full((Hkv, MAX_SEQ, hd), FILL, dtype=torch.float16, device=d))
    qb = gb.out("q_out", 2 * H * S * hd)
    args = (qkvb.ptr(), posb.ptr(), cosb.ptr(), sinb.ptr(), qb.ptr(), kcb.ptr(), vcb.ptr(), S, H, Hkv, hd, MAX_SEQ)
    if norm:
        qwb, kwb = gb.inp("q_norm_weight", qw), gb.inp("k_norm_weight", kw)
        L.check(L.lib().gq_qknorm_rope_cache_rows(*args, qwb.ptr(), kwb.ptr(), 1e-6, L.current_stream_ptr()), "gq_qknorm_rope_cache_rows")
    else:
        L.check(L.lib().gq_rope_cache_rows(*args, L.current_stream_ptr()), "gq_rope_cache_rows")
    gb.check()
    # the tensor expressions: q of every token (a position beyond the cache rotates with the last table row: its q is still written),
    # k / v of the tokens inside the cache
    q, k, v = qkv[:, :H * hd].view(S, H, hd), qkv[:, H * hd:(H + Hkv) * hd].view(S, Hkv, hd), qkv[:, (H + Hkv) * hd:].view(S, Hkv, hd)
    if norm:
        q, k = _qknorm(q, qw, 1e-6), _qknorm(k, kw, 1e-6)
    pc = pos.long().clamp(max=MAX_SEQ - 1)
    c, s = cos[pc].unsqueeze(1), sin[pc].unsqueeze(1)
    q_ref, k_ref = _rope(q, c, s).transpose(0, 1).contiguous(), _rope(k, c, s)
    q_got = qb.view(torch.float16, (H, S, hd))
    kc, vc = kcb.view(torch.float16, (Hkv, MAX_SEQ, hd)), vcb.view(torch.float16, (Hkv, MAX_SEQ, hd))
    inside = [i for i, p in enumerate(_positions(S)) if p < MAX_SEQ]
    rows = [_positions(S)[i] for i in inside]
    assert not torch.isnan(q_got).any()   # every q element was written
    if norm:
        assert float((q_got.float() - q_ref.float()).abs().max()) <= _spacing(q_ref)
        assert float((kc[:, rows].float() - k_ref[inside].transpose(0, 1).float()).abs().max()) <= _spacing(k_ref[inside])
    else:
        assert torch.equal(q_got.view(torch.int16), q_ref.view(torch.int16))
        assert torch.equal(kc[:, rows].contiguous().view(torch.int16), k_ref[inside].transpose(0, 1).contiguous().view(torch.int16))
    assert torch.equal(vc[:, rows].contiguous().view(torch.int16), v[inside].transpose(0, 1).contiguous().view(torch.int16))
    # cache rows no token addresses keep their fill
    keep = torch.ones(MAX_SEQ, dtype=torch.bool, device=d)
    keep[rows] = False
    assert bool((kc[:, keep] == FILL).all()) and bool((vc[:, keep] == FILL).all())
