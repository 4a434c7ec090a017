"""GPU, kernel level: gq_attn_decode_split_bias -- the decode attention launch that adds Qwen2's q / k / v bias in front of the rotation.

Exact.  The quantized linears round the GEMV result to fp16 and add the bias as ONE fp16 add (APLinear.forward: `output += bias`), so
gq_attn_decode_split_bias(qkv, bias) must equal gq_attn_decode_split(qkv + bias), the sum taken by torch in fp16, under torch.equal: on
the output, on the whole K cache and on the whole V cache.  The only difference between the two launches is that IEEE fp16 add; no
tolerance applies.  Values are drawn as in tests/test_qknorm_attn_gpu.py (N(0, 1) fp16 vectors and caches, rope base 1e6, max_seq 2048).
"""
import math

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HEAD_DIMS = (64, 128)
GEOMETRIES = ((8, 8), (8, 2), (28, 4), (14, 2))  # (28, 4), (14, 2): groups of 7, the Qwen2.5-7B and 0.5B ratios
SPLITS = (1, 4, 8)
MAX_SEQ = 2048
POSITIONS = (0, 1, 127, 128, 300, MAX_SEQ - 1)


def _inputs(hd, H, Hkv, seed):
    d = torch.device("cuda:0")
    g = torch.Generator(device=d)
    g.manual_seed(seed)
    from guidedquant_amd.model import rope_tables
    cos, sin = rope_tables(hd, MAX_SEQ, 1000000.0, d)
    kc = torch.randn(Hkv, MAX_SEQ, hd, device=d, generator=g).half()
    vc = torch.randn(Hkv, MAX_SEQ, hd, device=d, generator=g).half()
    return d, g, cos, sin, kc, vc


def _bias(H, Hkv, hd, d, g, k_scale=1.0):
    b = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g)
    b[H * hd:(H + Hkv) * hd] *= k_scale
    return b.half()


class _Launch:
    """both entry points over one set of buffers: returns (output, K cache, V cache) of a launch on fresh copies of the caches"""

    def __init__(self, hd, H, Hkv, cos, sin, kc0, vc0):
        self.hd, self.H, self.Hkv, self.cos, self.sin, self.kc0, self.vc0 = hd, H, Hkv, cos, sin, kc0, vc0
        self.ws = torch.zeros(H * max(SPLITS) * (hd + 2), dtype=torch.float32, device=kc0.device)

    def __call__(self, qkv, p, ns, bias=None):
        from guidedquant_amd import _lib
        L = _lib.lib()
        kc, vc = self.kc0.clone(), self.vc0.clone()
        out = torch.zeros(self.H * self.hd, dtype=torch.float16, device=kc.device)
        pos = torch.tensor([p], dtype=torch.int32, device=kc.device)
        args = (qkv.data_ptr(), pos.data_ptr(), self.cos.data_ptr(), self.sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), self.H, self.Hkv,
                self.hd, MAX_SEQ, 1.0 / math.sqrt(self.hd), ns, self.ws.data_ptr() if ns > 1 else None)
        if bias is None:
            _lib.check(L.gq_attn_decode_split(*args, _lib.current_stream_ptr()), "split")
        else:
            _lib.check(L.gq_attn_decode_split_bias(*args, bias.data_ptr(), _lib.current_stream_ptr()), "split_bias")
        torch.cuda.synchronize()
        return out, kc, vc


def _check_cases(hd, geometries, k_scale, seed0):
    n = 0
    for gi, (H, Hkv) in enumerate(geometries):
        d, g, cos, sin, kc0, vc0 = _inputs(hd, H, Hkv, seed0 + 100 * hd + gi)
        run = _Launch(hd, H, Hkv, cos, sin, kc0, vc0)
        keep = torch.ones(MAX_SEQ, dtype=torch.bool, device=d)
        for ns in SPLITS:
            for p in POSITIONS:
                qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
                bias = _bias(H, Hkv, hd, d, g, k_scale)
                want = run(qkv + bias, p, ns)  # (one fp16 add per element, by torch)
                got = run(qkv, p, ns, bias=bias)
                case = (hd, H, Hkv, ns, p, k_scale)
                assert torch.isfinite(want[0].float()).all(), case
                assert torch.equal(got[0], want[0]), ("output", case, (got[0].float() - want[0].float()).abs().max().item())
                assert torch.equal(got[1], want[1]), ("K cache", case)
                assert torch.equal(got[2], want[2]), ("V cache", case)
                # only cache row p is written, and it is written: the biased v, a k that is not the cached one
                keep.fill_(True)
                keep[p] = False
                assert torch.equal(got[1][:, keep], kc0[:, keep]) and torch.equal(got[2][:, keep], vc0[:, keep]), ("rows other than pos", case)
                v_ref = (qkv + bias)[(H + Hkv) * hd:].view(Hkv, hd)
                assert torch.equal(got[2][:, p], v_ref) and not torch.equal(got[1][:, p], kc0[:, p]), ("row pos", case)
                n += 1
    return n


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bias_form_equals_the_plain_form_on_the_biased_vector(hd):
    assert _check_cases(hd, GEOMETRIES, 1.0, 0) == len(GEOMETRIES) * len(SPLITS) * len(POSITIONS)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bias_form_with_a_large_k_bias(hd):
    """published Qwen2 k biases reach the tens: the k bias scaled by 30 (sums of magnitude ~100, fp16 spacing 2^-4)"""
    assert _check_cases(hd, GEOMETRIES, 30.0, 5000) == len(GEOMETRIES) * len(SPLITS) * len(POSITIONS)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_zero_bias_reproduces_the_plain_form(hd):
    H, Hkv = 28, 4
    d, g, cos, sin, kc0, vc0 = _inputs(hd, H, Hkv, 17 + hd)
    run = _Launch(hd, H, Hkv, cos, sin, kc0, vc0)
    zero = torch.zeros((H + 2 * Hkv) * hd, dtype=torch.float16, device=d)
    for ns in SPLITS:
        for p in POSITIONS:
            qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
            want, got = run(qkv, p, ns), run(qkv, p, ns, bias=zero)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (hd, ns, p)


@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bias_form_past_the_cache_is_nan_and_bad_arguments_are_refused(hd):
    from guidedquant_amd import _lib
    L = _lib.lib()
    H, Hkv = 8, 2
    d, g, cos, sin, kc0, vc0 = _inputs(hd, H, Hkv, 3)
    run = _Launch(hd, H, Hkv, cos, sin, kc0, vc0)
    qkv = torch.randn((H + 2 * Hkv) * hd, device=d, generator=g).half()
    bias = _bias(H, Hkv, hd, d, g)
    for ns in SPLITS:
        for p in (MAX_SEQ, MAX_SEQ + 5):
            out, kc, vc = run(qkv, p, ns, bias=bias)
            assert torch.isnan(out.float()).all() and torch.equal(kc, kc0) and torch.equal(vc, vc0), (hd, ns, p)
    # refused, not launched: a null bias, a bias that is not 16-byte aligned, a head_dim without a kernel
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.zeros(H * hd, dtype=torch.float16, device=d)
    pos = torch.tensor([0], dtype=torch.int32, device=d)

    def rc(head_dim, bias_ptr):
        return L.gq_attn_decode_split_bias(qkv.data_ptr(), pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), H, Hkv,
                                           head_dim, MAX_SEQ, 0.1, 1, None, bias_ptr, None)

    assert rc(hd, None) == _lib.GQ_EINVAL
    assert rc(hd, bias.data_ptr() + 2) == _lib.GQ_EINVAL
    assert rc(96, bias.data_ptr()) == _lib.GQ_ENOTSUP
    torch.cuda.synchronize()
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0) and not out.any()
