"""GPU, kernel level: the two launches that carry Qwen3's per-head q / k RMSNorm -- gq_attn_decode_split_qknorm (decode step) and
gq_qknorm_rope_cache_rows (prompt pass) -- against a torch restatement of modeling_qwen3.Qwen3Attention.forward with the same
rounding points (Qwen3RMSNorm: fp32 statistic, x * rsqrt(mean + eps) rounded to fp16, fp16 product with the weight; then
apply_rotary_pos_emb in fp16; scores / softmax / weighted sum in fp32, one fp16 rounding).

How the bounds were set.  The yardstick is what the kernels WITHOUT the norm (gq_attn_decode_split, gq_rope_cache_rows: the parent
commit's behaviour) deviate from the same restatement with the norm step removed, on the same inputs: `_measure(norm=False)`.  The
norm form is allowed twice the largest such deviation plus one fp16 spacing at the tensor's largest magnitude (the norm adds one
rsqrt, one reduction order and two fp16 roundings).  Measured on an MI355X (profiles/qwen3_fused_route.json carries the same figures):

                          without the norm (yardstick)            with the norm              bound at the worst case
  decode   k row          0 (bit-equal, 108 cases)                1.95e-3 (0.5 spacing)      0 + 3.9e-3
           output         4.88e-4 (2^-11; 71 of 108 cases > 0)    9.77e-4                    2 * 4.88e-4 + 1.95e-3
  prompt   q rows         0 (bit-equal, 16 cases)                 3.9e-3 (1.0 spacing)       0 + 3.9e-3
           k rows         0 (bit-equal)                           1.95e-3 (0.5 spacing)      0 + 3.9e-3
(values of magnitude 2 .. 6; "spacing" = one fp16 spacing at the largest magnitude of the case's reference tensor)
"""
import math

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# largest deviation of the kernels without the norm from the restatement without the norm, over all cases below (absolute, fp16 values
# of magnitude O(1)); the rotated k row and the copied v row are bit-equal, the attention output differs by summation order and __expf
BASE_DECODE_K_DEV = 0.0
BASE_DECODE_OUT_DEV = 2.0**-11  # 4.88e-4
BASE_PREFILL_Q_DEV = 0.0
BASE_PREFILL_K_DEV = 0.0

HEAD_DIMS = (64, 128)
GEOMETRIES = ((8, 8), (8, 2), (32, 8))
SPLITS = (1, 4, 8)
MAX_SEQ = 2048
POSITIONS = (0, 1, 127, 128, 300, MAX_SEQ - 1)
PREFILL_S = (1, 5, 128, 515)
PREFILL_START = 7


def _spacing(t):
    """one fp16 spacing at the largest magnitude of t"""
    m = float(t.float().abs().max())
    return 2.0**(math.floor(math.log2(m)) - 10) if m > 0 else 2.0**-24


def _rotate_half(x):
    return torch.cat((-x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]), dim=-1)


def _qknorm(x, w, eps):
    """Qwen3RMSNorm.forward on fp16 x [.., hd]"""
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * w


def _rope(x, cos, sin):  # x [.., hd] fp16, cos / sin [.., hd] fp16: three fp16-rounded operations
    return (x * cos) + (_rotate_half(x) * sin)


def _inputs(hd, H, Hkv, seed):
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(seed)
    from guidedquant_amd.model import rope_tables
    cos, sin = rope_tables(hd, MAX_SEQ, 1000000.0, d)
    kc = torch.randn(Hkv, MAX_SEQ, hd, device=d, generator=g).half()
    vc = torch.randn(Hkv, MAX_SEQ, hd, device=d, generator=g).half()
    qw = (1 + 0.3 * torch.randn(hd, device=d, generator=g)).half()
    kw = (1 + 0.3 * torch.randn(hd, device=d, generator=g)).half()
    return d, g, cos, sin, kc, vc, qw, kw


def _decode_reference(qkv, p, cos, sin, kc, vc, H, Hkv, hd, qw, kw, eps, norm):
    q, k, v = qkv[:H * hd].view(H, hd), qkv[H * hd:(H + Hkv) * hd].view(Hkv, hd), qkv[(H + Hkv) * hd:].view(Hkv, hd)
    if norm:
        q, k = _qknorm(q, qw, eps), _qknorm(k, kw, eps)
    q, k = _rope(q, cos[p], sin[p]), _rope(k, cos[p], sin[p])
    K = torch.cat([kc[:, :p], k.unsqueeze(1)], dim=1).float().repeat_interleave(H // Hkv, dim=0)  # [H, p + 1, hd]
    V = torch.cat([vc[:, :p], v.unsqueeze(1)], dim=1).float().repeat_interleave(H // Hkv, dim=0)
    s = torch.einsum("hd,htd->ht", q.float(), K) * (1.0 / math.sqrt(hd))
    out = torch.einsum("ht,htd->hd", torch.softmax(s, dim=-1), V).half()
    return k, v, out.reshape(-1)


def _measure_decode(norm):
    """every (head_dim, geometry, n_split, position): deviations of the written k row, the written v row and the output; returns
    {"k": (largest deviation, list of (deviation, spacing)), "out": .., "v_equal": bool}"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    eps = 1e-6
    res = dict(k=[], out=[], v_equal=True)
    for hd in HEAD_DIMS:
        for gi, (H, Hkv) in enumerate(GEOMETRIES):
            d, g, cos, sin, kc0, vc0, qw, kw = _inputs(hd, H, Hkv, 100 * hd + gi)
            ws = torch.zeros(H * max(SPLITS) * (hd + 2), dtype=torch.float32, device=d)
            out = torch.zeros(H * hd, dtype=torch.float16, device=d)
            for ns in SPLITS:
                for p in POSITIONS:
                    qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
                    pos = torch.tensor([p], dtype=torch.int32, device=d)
                    kc, vc = kc0.clone(), vc0.clone()
                    out.zero_()
                    args = (qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd,
                            MAX_SEQ, 1.0 / math.sqrt(hd), ns, ws.data_ptr() if ns > 1 else None)
                    if norm:
                        _lib.check(L.gq_attn_decode_split_qknorm(*args, qw.data_ptr(), kw.data_ptr(), eps, _lib.current_stream_ptr()), "qknorm")
                    else:
                        _lib.check(L.gq_attn_decode_split(*args, _lib.current_stream_ptr()), "split")
                    torch.cuda.synchronize()
                    k_ref, v_ref, o_ref = _decode_reference(qkv, p, cos, sin, kc0, vc0, H, Hkv, hd, qw, kw, eps, norm)
                    res["v_equal"] &= torch.equal(vc[:, p], v_ref)
                    # nothing but row p of the caches is written
                    keep = torch.ones(MAX_SEQ, dtype=torch.bool, device=d)
                    keep[p] = False
                    assert torch.equal(kc[:, keep], kc0[:, keep]) and torch.equal(vc[:, keep], vc0[:, keep]), (hd, H, Hkv, ns, p)
                    assert torch.isfinite(out.float()).all(), (hd, H, Hkv, ns, p)
                    res["k"].append(((kc[:, p].float() - k_ref.float()).abs().max().item(), _spacing(k_ref), (hd, H, Hkv, ns, p)))
                    res["out"].append(((out.float() - o_ref.float()).abs().max().item(), _spacing(o_ref), (hd, H, Hkv, ns, p)))
    return res


def _prefill_reference(qkv, start, cos, sin, H, Hkv, hd, qw, kw, eps, norm):
    S = qkv.shape[0]
    q, k, v = qkv[:, :H * hd].view(S, H, hd), qkv[:, H * hd:(H + Hkv) * hd].view(S, Hkv, hd), qkv[:, (H + Hkv) * hd:].view(S, Hkv, hd)
    if norm:
        q, k = _qknorm(q, qw, eps), _qknorm(k, kw, eps)
    c, s = cos[start:start + S].unsqueeze(1), sin[start:start + S].unsqueeze(1)
    return _rope(q, c, s).transpose(0, 1), _rope(k, c, s).transpose(0, 1), v.transpose(0, 1)  # [heads, S, hd]


def _measure_prefill(norm):
    from guidedquant_amd import _lib
    L = _lib.lib()
    eps = 1e-6
    res = dict(q=[], k=[], v_equal=True)
    for hd in HEAD_DIMS:
        for gi, (H, Hkv) in enumerate(((8, 2), (32, 8))):
            d, g, cos, sin, kc0, vc0, qw, kw = _inputs(hd, H, Hkv, 7 + 100 * hd + gi)
            for S in PREFILL_S:
                qkv = torch.randn(S, (H + 2 * Hkv) * hd, device=d, generator=g).half()
                pos = torch.arange(PREFILL_START, PREFILL_START + S, dtype=torch.int32, device=d)
                kc, vc = kc0.clone(), vc0.clone()
                q = torch.zeros(H, S, hd, dtype=torch.float16, device=d)
                args = (qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), S, H, Hkv, hd, MAX_SEQ)
                if norm:
                    _lib.check(L.gq_qknorm_rope_cache_rows(*args, qw.data_ptr(), kw.data_ptr(), eps, _lib.current_stream_ptr()), "qknorm rows")
                else:
                    _lib.check(L.gq_rope_cache_rows(*args, _lib.current_stream_ptr()), "rope rows")
                torch.cuda.synchronize()
                q_ref, k_ref, v_ref = _prefill_reference(qkv, PREFILL_START, cos, sin, H, Hkv, hd, qw, kw, eps, norm)
                rows = slice(PREFILL_START, PREFILL_START + S)
                res["v_equal"] &= torch.equal(vc[:, rows], v_ref)
                keep = torch.ones(MAX_SEQ, dtype=torch.bool, device=d)
                keep[rows] = False
                assert torch.equal(kc[:, keep], kc0[:, keep]) and torch.equal(vc[:, keep], vc0[:, keep]), (hd, H, Hkv, S)
                res["q"].append(((q.float() - q_ref.float()).abs().max().item(), _spacing(q_ref), (hd, H, Hkv, S)))
                res["k"].append(((kc[:, rows].float() - k_ref.float()).abs().max().item(), _spacing(k_ref), (hd, H, Hkv, S)))
    return res


def _worst(rows):
    return max(r[0] for r in rows)


def test_decode_attention_with_qk_norm_matches_the_restatement():
    base = _measure_decode(norm=False)
    got = _measure_decode(norm=True)
    print("decode, no norm (yardstick): k row %.4e  out %.4e   with norm: k row %.4e  out %.4e" %
          (_worst(base["k"]), _worst(base["out"]), _worst(got["k"]), _worst(got["out"])))
    assert base["v_equal"] and got["v_equal"]  # v is copied, untouched
    # the yardstick itself has not moved from what the constants record
    assert _worst(base["k"]) <= BASE_DECODE_K_DEV and _worst(base["out"]) <= BASE_DECODE_OUT_DEV
    for dev, sp, case in got["k"]:
        assert dev <= 2 * BASE_DECODE_K_DEV + sp, ("k row", case, dev, sp)
    for dev, sp, case in got["out"]:
        assert dev <= 2 * BASE_DECODE_OUT_DEV + sp, ("out", case, dev, sp)


def test_decode_attention_with_qk_norm_uses_both_weights():
    """a swapped or dropped weight moves the k row by far more than the bound"""
    from guidedquant_amd import _lib
    L = _lib.lib()
    hd, H, Hkv, p = 128, 8, 2, 5
    d, g, cos, sin, kc, vc, qw, kw = _inputs(hd, H, Hkv, 9)
    qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
    pos = torch.tensor([p], dtype=torch.int32, device=d)
    out = torch.zeros(H * hd, dtype=torch.float16, device=d)
    outs = []
    for a, b in ((qw, kw), (kw, qw)):
        _lib.check(L.gq_attn_decode_split_qknorm(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv,
                                                 hd, MAX_SEQ, 1.0 / math.sqrt(hd), 1, None, a.data_ptr(), b.data_ptr(), 1e-6, _lib.current_stream_ptr()), "qknorm")
        torch.cuda.synchronize()
        outs.append((kc[:, p].clone(), out.clone()))
    assert (outs[0][0].float() - outs[1][0].float()).abs().max().item() > 0.1
    assert (outs[0][1].float() - outs[1][1].float()).abs().max().item() > 1e-2


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_decode_attention_with_qk_norm_past_the_cache_is_nan(hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv = 8, 2
    d, g, cos, sin, kc0, vc0, qw, kw = _inputs(hd, H, Hkv, 3)
    qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
    ws = torch.zeros(H * 8 * (hd + 2), dtype=torch.float32, device=d)
    for ns in SPLITS:
        for p in (MAX_SEQ, MAX_SEQ + 5):
            kc, vc = kc0.clone(), vc0.clone()
            out = torch.zeros(H * hd, dtype=torch.float16, device=d)
            pos = torch.tensor([p], dtype=torch.int32, device=d)
            _lib.check(L.gq_attn_decode_split_qknorm(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H,
                                                     Hkv, hd, MAX_SEQ, 1.0 / math.sqrt(hd), ns, ws.data_ptr() if ns > 1 else None, qw.data_ptr(), kw.data_ptr(),
                                                     1e-6, _lib.current_stream_ptr()), "qknorm")
            torch.cuda.synchronize()
            assert torch.isnan(out.float()).all() and torch.equal(kc, kc0) and torch.equal(vc, vc0)
    # bad arguments are refused, not launched
    assert L.gq_attn_decode_split_qknorm(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, 96,
                                         MAX_SEQ, 0.1, 1, None, qw.data_ptr(), kw.data_ptr(), 1e-6, None) == _lib.GQ_ENOTSUP
    assert L.gq_attn_decode_split_qknorm(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv, hd,
                                         MAX_SEQ, 0.1, 1, None, None, kw.data_ptr(), 1e-6, None) != 0


def test_prompt_rows_with_qk_norm_match_the_restatement():
    base = _measure_prefill(norm=False)
    got = _measure_prefill(norm=True)
    print("prompt rows, no norm (yardstick): q %.4e  k %.4e   with norm: q %.4e  k %.4e" %
          (_worst(base["q"]), _worst(base["k"]), _worst(got["q"]), _worst(got["k"])))
    assert base["v_equal"] and got["v_equal"]
    assert _worst(base["q"]) <= BASE_PREFILL_Q_DEV and _worst(base["k"]) <= BASE_PREFILL_K_DEV
    for dev, sp, case in got["q"]:
        assert dev <= 2 * BASE_PREFILL_Q_DEV + sp, ("q", case, dev, sp)
    for dev, sp, case in got["k"]:
        assert dev <= 2 * BASE_PREFILL_K_DEV + sp, ("k", case, dev, sp)
