"""GPU: widening the fused sampler to 262144 logits moved nothing at 131072 and below.

tests/golden/sampler_narrow_draws.npz holds 256 tokens per case, drawn at 128256 logits (the benchmark's vocabulary) for
k in {1, 32, 50} x T in {0, 0.8} x top_p in {1, 0.9} through gq_sample_topk_p with one seed and one starting counter.  It was recorded
on an MI355X from the library of commit a8d2596 ("One dispatcher for the AP GEMV: policy moves to ap_dispatch.hip"), the last one
whose sampler stopped at 131072: that commit's guidedquant_amd/csrc built into a directory of its own, GQ_LIB_PATH pointed at its
libgq_hip.so, and

    GQ_LIB_PATH=<that library> python tests/test_sampler_narrow_unchanged_gpu.py <output .npz>

run on the GPU (`record` below).  The logits come from the integer formula of `_logits`, not from a generator, so the fixture holds
the tokens only.  The test asserts that the built library draws exactly these tokens."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sampler_narrow_draws.npz")
V, N_DRAWS, SEED, COUNTER0 = 128256, 256, 0x5EED, 4096
CASES = [(k, T, p) for k in (1, 32, 50) for T in (0.0, 0.8) for p in (1.0, 0.9)]


def _logits():
    """fp16 logits from integer arithmetic alone: two 16-bit halves of a hashed index, added -- a triangular distribution over
    [-16, 16) in steps of 1/4096, whose upper tail rounds to fp16 values 1/128 apart (ties among the candidates included)"""
    i = np.arange(V, dtype=np.uint64)
    u = (i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)
    u ^= u >> np.uint64(15)
    u = (u * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    u ^= u >> np.uint64(13)
    s = (u & np.uint64(0xFFFF)).astype(np.int64) + (u >> np.uint64(16)).astype(np.int64) - 65535
    return (s.astype(np.float32) / np.float32(4096.0)).astype(np.float16)  # (both steps are exact or a single rounding to nearest)


def _key(k, T, p):
    return "k%d_T%s_p%s" % (k, T, p)


def _draw_all():
    from guidedquant_amd import _lib
    L = _lib.lib()
    d = torch.device("cuda:0")
    logits = torch.from_numpy(_logits()).to(d)
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=d)  # noqa: E731
    wv, wi = z(128 * 64, torch.float32), z(128 * 64, torch.int32)
    out = {}
    for k, T, p in CASES:
        ctr, tok, pos, nt = (z(1, torch.int32) for _ in range(4))
        ctr.fill_(COUNTER0)
        seq = torch.full((N_DRAWS + 1, ), -1, dtype=torch.int32, device=d)
        for _ in range(N_DRAWS):
            _lib.check(L.gq_sample_topk_p(logits.data_ptr(), V, k, p, T, SEED, ctr.data_ptr(), wv.data_ptr(), wi.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                                          nt.data_ptr(), None, seq.data_ptr(), seq.numel(), None, None, 0, None, _lib.current_stream_ptr()), "gq_sample_topk_p")
        torch.cuda.synchronize()
        assert int(pos.item()) == N_DRAWS and int(ctr.item()) == COUNTER0 + N_DRAWS
        out[_key(k, T, p)] = seq[1:].cpu().numpy().astype(np.int32)
    return out


def record(path):
    """writes the fixture from whatever library GQ_LIB_PATH names (the parent commit's, see the module docstring)"""
    np.savez_compressed(path, **_draw_all())


def test_logits_formula_gives_a_spread_tail_with_ties():
    """(what makes the fixture worth having: the 64 largest logits are neither all equal nor all distinct)"""
    x = np.sort(_logits().astype(np.float32))[::-1][:64]
    assert 8 < len(np.unique(x)) < 64 and x[0] < 16.0


def test_draws_at_128256_logits_equal_the_recorded_ones():
    want = np.load(FIXTURE)
    assert sorted(want.files) == sorted(_key(*c) for c in CASES)
    got = _draw_all()
    for c in CASES:
        w, g = want[_key(*c)], got[_key(*c)]
        assert w.shape == (N_DRAWS, ) and w.min() >= 0 and w.max() < V
        assert np.array_equal(w, g), (c, int((w != g).sum()), w[:8], g[:8])
    # (the recorded draws are not degenerate: the sampled cases spread over their candidates, the greedy ones repeat one token)
    assert len(set(want[_key(50, 0.8, 1.0)].tolist())) > 8 and len(set(want[_key(50, 0.0, 1.0)].tolist())) == 1


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    record(sys.argv[1])
    print("recorded", sys.argv[1])
