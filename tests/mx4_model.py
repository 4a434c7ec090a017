"""The MXFP4 KV cache's write rule and dequantisation (include/gq_hip.h) restated in numpy float64, independent of model.mxfp4_quantize:
the exponent from frexp (no logarithm), the code as the nearest of the 8 e2m1 magnitudes with a tie to the even code."""
import numpy as np

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
BLOCK = 32


def quantize(x16):
    """np.float16 [.., head_dim] -> (codes uint8 [.., head_dim / 2], exponent bytes uint8 [.., head_dim / 32])"""
    xb = x16.reshape(x16.shape[:-1] + (-1, BLOCK))
    x = np.abs(xb.astype(np.float64))
    finite = np.isfinite(x).all(-1)
    amax = np.where(finite, np.where(np.isfinite(x), x, 0.0).max(-1), 0.0)
    m, ex = np.frexp(amax / 6.0)  # amax / 6 = m 2^ex, 0.5 <= m < 1: ceil(log2) = ex, or ex - 1 at m = 0.5
    e = np.where(amax > 0, np.clip(np.where(m == 0.5, ex - 1, ex), -15, 13), -15)
    e = np.where(finite, e, 13)  # (a block with an Inf or a NaN: its codes are taken at the largest exponent)
    y = x * np.exp2(-e.astype(np.float64))[..., None]
    d = np.abs(np.where(np.isfinite(y), y, 7.0)[..., None] - MAGS)
    lo = d.argmin(-1)  # (the first, hence the lower, of two equally near codes)
    tie = np.take_along_axis(d, np.minimum(lo + 1, 7)[..., None], -1)[..., 0] == np.take_along_axis(d, lo[..., None], -1)[..., 0]
    code = np.where(tie & (lo < 7) & (lo % 2 == 1), lo + 1, lo)
    code = (code | ((xb.view(np.uint16) >> 15) << 3)).astype(np.uint8).reshape(x16.shape)
    return code[..., 0::2] | (code[..., 1::2] << 4), np.where(finite, e + 127, 0xFF).astype(np.uint8)


def dequant(codes, exps):
    """float64 [.., head_dim]: e2m1(code) * 2^(byte - 127), NaN in a block with the byte 0xFF"""
    nib = np.stack((codes & 0xF, codes >> 4), -1).reshape(codes.shape[:-1] + (-1, BLOCK))
    scale = np.where(exps == 0xFF, np.nan, np.exp2(exps.astype(np.float64) - 127))
    return (np.where(nib & 8, -1.0, 1.0) * MAGS[nib & 7] * scale[..., None]).reshape(codes.shape[:-1] + (-1,))


def error_bound(x, exps):
    """the stated bound on |x - deq| of a finite x with |x| <= 6 * 2^e: half the step of the binade of the e2m1 grid that x / 2^e falls in
    -- 2^e from 4 * 2^e on, 2^(e - 1) from 2 * 2^e on, 2^(e - 2) below"""
    s = np.repeat(np.exp2(exps.astype(np.float64) - 127), BLOCK, -1)
    return np.where(np.abs(x) >= 4 * s, s, np.where(np.abs(x) >= 2 * s, s / 2, s / 4))
