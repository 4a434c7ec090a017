"""The opt-in int8 lm_head (weight-only, one scale per output row): the host side.

`quantize_rows_int8` is the one-off work per model; the launch that reads its result is gq_dense_gemv_i8 (csrc/head_q8.hip,
include/gq_hip.h), chosen by `Transformer.set_lm_head_dtype("int8")`.  The default head stays fp16, as in the reference.
"""
import torch


def lm_head_dtype_name(lm_head_dtype) -> str:
    """None / "fp16" -> "fp16" (the head as the checkpoint holds it: the default), "int8" -> "int8" (codes + an fp32 scale per row)"""
    name = "fp16" if lm_head_dtype is None else str(lm_head_dtype)
    if name not in ("fp16", "int8"):
        raise ValueError(f"lm_head_dtype={lm_head_dtype!r}: None, 'fp16' or 'int8'")
    return name


def quantize_rows_int8(W: torch.Tensor):
    """W fp16 [N, K] -> (q int8 [N, K] contiguous, scale fp32 [N]), symmetric, per row:
        scale[n] = fp32(max_k |W[n][k]|) / 127                                        (an fp32 division)
        q[n][k]  = clamp(round_half_even(fp32(W[n][k]) / scale[n]), -127, 127)
    A row of zeros gets scale 1 and q 0; a non-finite weight raises ValueError.  Plain torch ops: the CPU and the GPU give the same
    tensors.  |scale * q - W| <= scale / 2 up to the rounding of the fp32 quotient."""
    if W.dim() != 2 or W.dtype != torch.float16:
        raise ValueError(f"quantize_rows_int8: an fp16 [N, K] tensor, not {W.dtype} {tuple(W.shape)}")
    if not bool(torch.isfinite(W).all()):
        raise ValueError("quantize_rows_int8: the weight holds a NaN or an Inf")
    N, K = W.shape
    q = torch.empty(N, K, dtype=torch.int8, device=W.device)
    scale = torch.empty(N, dtype=torch.float32, device=W.device)
    for r0 in range(0, N, ROWS):  # (row blocks: the fp32 intermediates of a 128256 x 4096 head stay at 0.25 GB instead of 4)
        w = W[r0:r0 + ROWS].detach().float()
        absmax = w.abs().amax(dim=1)
        # (a tensor divisor: a Python scalar would make the GPU multiply by the rounded reciprocal, another scale than the CPU's)
        s = torch.where(absmax > 0, absmax / torch.full_like(absmax, 127.0), torch.ones_like(absmax))
        scale[r0:r0 + ROWS] = s
        q[r0:r0 + ROWS] = torch.round(w / s[:, None]).clamp_(-127, 127).to(torch.int8)  # (torch.round: half to even)
    return q, scale


ROWS = 8192  # rows per block of quantize_rows_int8
