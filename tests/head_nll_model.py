"""Host model of the scoring head gq_head_nll (csrc/head_nll.hip; a plain helper module): numpy, float64.

The kernel's contract has one rounding point -- logit = fp16(sum_k xn[k] W[v][k]) -- and everything behind it is a function of those
fp16 values.  The model therefore TAKES the fp16 logits (widened to float64) and computes
    lse[s]     = log sum_v exp(logit[s][v])          float64, max subtracted
    logprob[s] = logit[s][target[s]] - lse[s]        0.0 for a negative target
    top1[s]    = np.argmax(logit[s])                 first occurrence: the lowest id among the largest
`logits16` makes those logits from the inputs with a float64 product; the input families of the tests live here so that the CPU test of
the premises and the GPU test of the kernel draw the same numbers.
"""
import numpy as np

# the shapes (S, V, D) of the exact family, and the largest error of torch's fp32 cross_entropy / logsumexp against float64 on their
# logits (measured on the CPU: 9.55e-7, at (129, 4104, 512); test_head_nll_model_cpu.py asserts it) -- the kernel's bound is 4 x this
EXACT_SHAPES = [(1, 40, 64), (15, 128, 64), (16, 129, 192), (63, 2087, 256), (64, 2088, 256), (65, 2088, 256), (129, 4104, 512)]
REF_ERR = 9.6e-7


def logits16(xn, W):
    """fp16(xn W^T) from a float64 product, as float64 [S, V]"""
    with np.errstate(over="ignore"):
        return (xn.astype(np.float64) @ W.astype(np.float64).T).astype(np.float16).astype(np.float64)


def model(logits, target):
    """(lse, logprob, top1) of float64 logits [S, V] and int targets [S]"""
    logits = np.asarray(logits, dtype=np.float64)
    target = np.asarray(target).astype(np.int64)
    m = logits.max(axis=1)
    lse = m + np.log(np.exp(logits - m[:, None]).sum(axis=1))
    rows = np.arange(logits.shape[0])
    lp = np.where(target >= 0, logits[rows, np.maximum(target, 0)] - lse, 0.0)
    return lse, lp, np.argmax(logits, axis=1).astype(np.int64)


def ulp16(x):
    """the spacing of fp16 at |x| (normal range; 2^-24 below it)"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0**-14)))
    return 2.0**(e - 10)


def exact_case(S, V, D, seed=0):
    """xn in {-1, 0, 1} / 4, W in {-2 .. 2} / 8 (fp16): every product is a multiple of 1 / 32 and every partial sum is exact in fp32 in
    any order (|sum| <= D / 16, a multiple of 2^-5: under 2^24 steps), and |logit| <= 32 keeps the multiples of 1 / 32 exact in fp16"""
    assert D <= 512
    r = np.random.RandomState(1000 + seed)
    xn = (r.randint(-1, 2, size=(S, D)) / 4.0).astype(np.float16)
    W = (r.randint(-2, 3, size=(V, D)) / 8.0).astype(np.float16)
    return xn, W


def roundoff_case(S, V, D, seed=0):
    """xn = randn, W = 0.05 randn (fp16): logits of a few units whose fp16 rounding depends on the summation order"""
    r = np.random.RandomState(2000 + seed)
    return r.randn(S, D).astype(np.float16), (0.05 * r.randn(V, D)).astype(np.float16)


def targets(S, V, splits_edges, seed=0):
    """int32 [S]: column 0, column V - 1, -1 and the first and last column of every split range in `splits_edges` ([(lo, hi)], hi
    exclusive) on the leading rows, random columns on the rest.  Where S is smaller than that list, `seed` rotates which ones are in."""
    r = np.random.RandomState(3000 + seed)
    t = r.randint(0, V, size=S).astype(np.int32)
    special = [0, V - 1, -1]
    for lo, hi in splits_edges:
        if lo < hi:
            special += [lo, hi - 1]
    for i in range(min(S, len(special))):
        t[i] = special[(i + seed) % len(special)]
    return t


BV = 128  # vocabulary rows per tile of the kernel (csrc/head_nll.hip)


def split_ranges(V, splits):
    """the column ranges [(lo, hi)] the kernel's `splits` >= 1 vocabulary splits cover: whole tiles, ceil(tiles / splits) each"""
    ntiles = (V + BV - 1) // BV
    tps = (ntiles + splits - 1) // splits
    return [(min(s * tps * BV, V), min((s + 1) * tps * BV, V)) for s in range(splits)]
