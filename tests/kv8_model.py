"""Host model of the fp8 (e4m3) KV cache (include/gq_hip.h, "The fp8 KV cache"): the write rule, the read rule and the byte codes the
tests plant.  Plain torch on the CPU: no GPU, no library.

  write   code  = fp8_rne(clamp(float(x16) * inv, -448, 448))       `quantize`
  read    value = float(code) * scale                               `dequant` (a 256-entry table: exact)
"""
import torch

NAN_CODE, MAX_CODE, ONE_CODE = 0x7F, 0x7E, 0x38  # NaN, 448, 1.0
HEADS = [(8, 2, 64), (4, 4, 128), (6, 2, 128)]   # (n_head, n_kv_head, head_dim) of the kernel tests

TABLE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()  # code -> value (0x7f / 0xff: NaN)


def quantize(x16, inv):
    """fp16 values -> uint8 codes; inv: fp32, broadcast against x16"""
    assert x16.dtype == torch.float16
    return (x16.float().cpu() * inv.float().cpu()).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def dequant(codes, scale=None, dtype=torch.float32):
    """uint8 codes [Hkv, n, hd] -> values; scale: fp32 [Hkv] or None (1.0).  The product is taken in `dtype`'s arithmetic from the fp32 scale."""
    v = TABLE.to(codes.device)[codes.long()].to(dtype)
    return v if scale is None else v * scale.to(codes.device).to(dtype)[:, None, None]


def random_codes(shape, gen, max_exp_code=0x7E):
    """uniform random bytes without the two NaN codes; magnitudes up to `max_exp_code` (0x7e: 448)"""
    mag = torch.randint(0, max_exp_code + 1, shape, generator=gen, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int32) << 7
    return (mag | sign).to(torch.uint8)


def stale_rows(n, hd):
    """rows an earlier sequence left behind the position: whole rows of NaN (0x7f) and 448 (0x7e), alternating"""
    r = torch.tensor([NAN_CODE, MAX_CODE], dtype=torch.uint8)[torch.arange(n) % 2]
    return r[None, :, None].expand(1, n, hd)


def scale_sets(Hkv):
    """name -> (k_scale, v_scale) fp32 [Hkv]: ones, powers of two mixed per head (2^-3 | 1 for K, 2^2 | 2^-1 for V), arbitrary"""
    i = torch.arange(Hkv)
    return {
        "ones": (torch.ones(Hkv), torch.ones(Hkv)),
        "pow2": (torch.where(i % 2 == 0, 2.0**-3, 1.0).float(), torch.where(i % 2 == 0, 4.0, 0.5).float()),
        "free": (torch.where(i % 2 == 0, 0.0037, 0.0113).float(), torch.where(i % 2 == 0, 0.37, 2.9).float()),
    }
