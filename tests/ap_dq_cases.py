"""The launches whose fp16 output words tests/golden/ap_dq_outputs.json records (tools/record_ap_dq_outputs.py) and
tests/test_ap_dq_parent_gpu.py replays: the decode-to-fp16 matrix-core GEMV (csrc/ap_dq.hip) at every bit width, over the shapes at
which its code takes another path, in every launch form.  Seeded inputs, every buffer through tests/guarded.py, the route asserted."""
import os

import numpy as np

from ap_helpers import run_fused_guarded

EPS = 1e-5
BITS = [2, 3, 4]
SHAPES = [(16, 1024),    # smallest served
          (18, 1024),    # ragged second row group, even N for the pairs
          (40, 4096),    # the QT = 32 instance
          (40, 14336),   # QT = 112, 28 units: the eight-at-a-time tail of the K-split sum and its remainder
          (34, 17408),   # 544 staging items on 512 staging threads: the re-read path, general instance
          (16, 32768)]   # widest row
FORMS = ["plain", "residual", "rmsnorm", "rmsnorm_pairs", "silu_prologue"]
CASES = [f"b{bits}_{N}x{K}_{form}" for bits in BITS for N, K in SHAPES for form in FORMS]


class dq_everywhere:
    """fast mode with every served launch sent to the dq kernel (GQ_DQ=7, GQ_DQ_MIN_MWEIGHTS=0)"""

    def __enter__(self):
        from guidedquant_amd import _lib
        self.L = _lib.lib()
        os.environ["GQ_DQ"] = "7"
        os.environ["GQ_DQ_MIN_MWEIGHTS"] = "0"
        self.L.gq_reset_env_cache()
        self.L.gq_set_ap_mode(0)

    def __exit__(self, *exc):
        os.environ.pop("GQ_DQ", None)
        os.environ.pop("GQ_DQ_MIN_MWEIGHTS", None)
        self.L.gq_reset_env_cache()
        self.L.gq_set_ap_mode(-1)


def run(name):
    """the output of one case as hex: four digits per fp16 word, in row order.  Call inside dq_everywhere."""
    from guidedquant_amd import pack
    b, shape, form = name.split("_", 2)
    bits, (N, K) = int(b[1:]), map(int, shape.split("x"))
    seed = 1000 * bits + 7 * N + K + FORMS.index(form)
    rng = np.random.default_rng(seed)
    q = pack.random_planes(N, K, bits, seed=seed)
    lut = np.sort(rng.normal(0, 0.02, (N, 1 << bits)).astype(np.float16), axis=1)
    x = rng.normal(0, 1, 2 * K if form == "silu_prologue" else K)
    x[rng.choice(K, 4, replace=False)] *= 30.0  # massive channels
    x = x.astype(np.float16)
    kw = {}
    if form == "residual":
        kw = dict(residual=rng.normal(0, 1, N).astype(np.float16), flags=1)
    elif form in ("rmsnorm", "rmsnorm_pairs"):
        kw = dict(norm_weight=(1 + 0.1 * rng.normal(0, 1, K)).astype(np.float16), eps=EPS)
        if form == "rmsnorm_pairs":
            kw.update(flags=4, out_elems=N // 2)
    elif form == "silu_prologue":
        kw = dict(flags=2)
    out = run_fused_guarded(x, q, lut, bits, expect="dq", **kw)
    assert np.isfinite(out).all(), name
    return out.view(np.uint16).astype(">u2").tobytes().hex()
