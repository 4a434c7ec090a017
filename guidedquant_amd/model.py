"""gpt-fast style Transformer -- the caller of the quantized linears, mirroring inference/model.py of the reference.

Same public surface: `ModelArgs`, `transformer_configs`, `KVCache`, `Transformer.from_name(dtype, name, linear_class,
linear_kwargs, halve_layers, fuse_linears)`, `setup_caches`, `forward(idx, input_pos)`; same module tree and state-dict
keys (`layers.{i}.attention.{wqkv,wo}`, `layers.{i}.feed_forward.{w1w3,w2}`, `..._layernorm.weight`, `norm.weight`,
`output.weight`, `tok_embeddings.weight`; inference/sqllm_llama_convert_fuse.py:73-116), so a
`converted_pytorch_model.bin` written for the reference loads unchanged.

Three execution paths:
  * `forward(idx, input_pos)`: plain PyTorch ops around `linear_class` modules -- the reference's semantics
    (model.py:121-130, 151-166, 206-266), used for prefill, for any linear class, and as the on-device statement the
    fused path is tested against.  RoPE is re-stated here (`rope_tables`): the reference imports
    `ROPE_INIT_FUNCTIONS["default"]`, which the installed transformers no longer has (model.py:15,353).
  * `decode_native(tok, pos)`: one bs=1 decode step as 5 HIP launches per layer through the C ABI
    (RMSNorm -> wqkv | RoPE + KV update + attention | wo + residual | RMSNorm -> w1w3 | SiLU*up -> w2 + residual),
    an embedding lookup and a fused final-norm + lm_head GEMV: no allocation, no host sync, token / position read
    from device memory, so the whole step is hipGraph-capturable (generate.py).  Its host side is native_step.py.
  * `prefill_native(idx, input_pos)` / `score_native(idx)`: the prompt pass (seq_len > 1, batch 1) with the element-wise steps between
    the linears as one HIP launch each and the attention as a HIP kernel or SDPA; logits, or log-probabilities through the scoring head.
    Its host side is native_prompt.py; `mask_rows`, `prefill_chunks` and `_sdpa_gqa` are re-exported from there.

Block layouts: Llama's, and with `ModelArgs.head_dim` / `qk_norm` Mistral's and Qwen3's (RMSNorm over head_dim on every q and k head in
front of the rotation, modeling_qwen3.Qwen3Attention.forward): in `Attention.forward` for the module path, inside the attention launch
(gq_attn_decode_split_qknorm) and the prompt pass's RoPE launch (gq_qknorm_rope_cache_rows) for the HIP path.  With `attn_bias` Qwen2's /
Qwen2.5's (modeling_qwen2.Qwen2Attention: a bias on q_proj / k_proj / v_proj, none on o_proj or the MLP): the quantized linear adds it in the
module path and the prompt pass, the attention launch (gq_attn_decode_split_bias) in the decode step.

Model table: the reference's entries (model.py:53-61) plus Llama-3.2-1B-Instruct and Llama-3.3-70B-Instruct, which
BASELINE.json's configs name and the reference table lacks.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
from torch import Tensor
from torch.nn import functional as F

from . import _lib, native_prompt, native_step
from .native_prompt import _SDPA_GQA, _sdpa_gqa, mask_rows, prefill_chunks  # noqa: F401  (the prompt pass's own; importable from here as they always were)


def find_multiple(n: int, k: int) -> int:
    if n % k == 0:
        return n
    return n + k - (n % k)


@dataclass
class ModelArgs:
    block_size: int = 2048
    vocab_size: int = 32000
    n_layer: int = 32
    n_head: int = 32
    dim: int = 4096
    intermediate_size: int = None
    n_local_heads: int = -1
    head_dim: Optional[int] = None  # None: dim // n_head (Llama); Qwen3 / Mistral configs carry their own
    rope_base: float = 10000
    norm_eps: float = 1e-5
    rope_scaling: Optional[dict] = None
    model_name: Optional[str] = None
    qk_norm: bool = False  # Qwen3: RMSNorm over head_dim on every q and k head in front of the rotation
    attn_bias: bool = False  # Qwen2 / Qwen2.5: q / k / v linears carry a bias (wo and the MLP do not)
    # sliding-window layers (Mistral; Qwen2 / Qwen3 with use_sliding_window): per layer None (the whole context) or W >= 1 -- the query at
    # position p attends the keys (p - W, p].  None: every layer attends the whole context.
    layer_windows: Optional[tuple] = None

    def __post_init__(self):
        if self.n_local_heads == -1:
            self.n_local_heads = self.n_head
        if self.intermediate_size is None:
            hidden_dim = 4 * self.dim
            n_hidden = int(2 * hidden_dim / 3)
            self.intermediate_size = find_multiple(n_hidden, 256)
        if self.head_dim is None:
            assert self.dim % self.n_head == 0
            self.head_dim = self.dim // self.n_head
        if self.layer_windows is not None:
            self.layer_windows = tuple(None if w is None else int(w) for w in self.layer_windows)
            assert len(self.layer_windows) == self.n_layer and all(w is None or w >= 1 for w in self.layer_windows), self.layer_windows
            if all(w is None for w in self.layer_windows):
                self.layer_windows = None

    @classmethod
    def from_name(cls, name: str):
        assert name in transformer_configs, f"Unknown model name: {name}, available: {transformer_configs.keys()}"
        return cls(**transformer_configs[name])


transformer_configs = {
    "meta-llama/Meta-Llama-3-8B": dict(model_name="Meta-Llama-3-8B", block_size=8192, n_layer=32, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, rope_base=500000),
    "meta-llama/Meta-Llama-3-8B-Instruct": dict(model_name="Meta-Llama-3-8B-Instruct", block_size=8192, n_layer=32, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, rope_base=500000),
    "meta-llama/Meta-Llama-3.1-8B": dict(model_name="Meta-Llama-3.1-8B", block_size=8192, n_layer=32, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, rope_base=500000),
    "meta-llama/Meta-Llama-3.1-8B-Instruct": dict(model_name="Meta-Llama-3.1-8B-Instruct", block_size=8192, n_layer=32, n_head=32, n_local_heads=8, dim=4096, intermediate_size=14336, vocab_size=128256, rope_base=500000),
    "meta-llama/Llama-2-7b": dict(model_name="Llama-2-7b", block_size=4096, n_layer=32, n_head=32, n_local_heads=32, dim=4096, intermediate_size=11008, vocab_size=32000, rope_base=10000),
    "meta-llama/Llama-2-13b": dict(model_name="Llama-2-13b", block_size=4096, n_layer=40, n_head=40, n_local_heads=40, dim=5120, intermediate_size=13824, vocab_size=32000, rope_base=10000),
    "meta-llama/Llama-2-70b": dict(model_name="Llama-2-70b", block_size=4096, n_layer=80, n_head=64, n_local_heads=8, dim=8192, intermediate_size=28672, vocab_size=32000, rope_base=10000),
    # not in the reference table: public HF configs, with the llama3 rope_scaling their config.json
    # carries (the reference's own 3.1 entries above have none and are kept as the reference has them)
    "meta-llama/Llama-3.2-1B-Instruct": dict(model_name="Llama-3.2-1B-Instruct", block_size=8192, n_layer=16, n_head=32, n_local_heads=8, dim=2048, intermediate_size=8192, vocab_size=128256, rope_base=500000,
                                             rope_scaling=dict(rope_type="llama3", factor=32.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)),
    "meta-llama/Llama-3.3-70B-Instruct": dict(model_name="Llama-3.3-70B-Instruct", block_size=8192, n_layer=80, n_head=64, n_local_heads=8, dim=8192, intermediate_size=28672, vocab_size=128256, rope_base=500000,
                                              rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=8192)),
    # Qwen3 dense (QK-norm, head_dim of its own).  The figures restate the public config from memory and could not be checked
    # offline: they serve as a shape set for --random_init runs and timing (tools/qwen3_decode_timing.py), not as a loader's truth --
    # a checkpoint's own config.json goes through hf_loader.model_args_from_hf_config.
    "Qwen/Qwen3-8B": dict(model_name="Qwen3-8B", block_size=8192, n_layer=36, n_head=32, n_local_heads=8, dim=4096, head_dim=128, intermediate_size=12288,
                          vocab_size=151936, rope_base=1000000, norm_eps=1e-6, qk_norm=True),
    # Qwen2.5 dense (q / k / v bias).  Restated from memory like the Qwen3 entry: a shape set for --random_init runs and timing.
    "Qwen/Qwen2.5-7B": dict(model_name="Qwen2.5-7B", block_size=8192, n_layer=28, n_head=28, n_local_heads=4, dim=3584, head_dim=128,
                            intermediate_size=18944, vocab_size=152064, rope_base=1000000, norm_eps=1e-6, attn_bias=True),
}


def rope_inv_freq(head_dim: int, base: float, rope_scaling: Optional[dict], device):
    """fp32 inverse frequencies of the rotary embedding for the `rope_scaling` section of a Llama config.json:
    None / "default": base^-(2i/d);  "linear": the same divided by `factor`;  "llama3" (Llama-3.1 / 3.2 / 3.3 checkpoints,
    inference/model.py:288-305 `apply_rope_scaling`): components whose wavelength exceeds original_max_position_embeddings /
    low_freq_factor are divided by `factor`, those shorter than original / high_freq_factor are kept, the band between is
    blended linearly in original / wavelength.  Any other type raises: decoding with the wrong frequencies would differ
    from the HF path that produced and evaluated the checkpoint at every position, silently."""
    inv_freq = 1.0 / (base**(torch.arange(0, head_dim, 2, dtype=torch.int64).to(dtype=torch.float32, device=device) / head_dim))
    if not rope_scaling:
        return inv_freq
    kind = rope_scaling.get("rope_type", rope_scaling.get("type", "default"))
    if kind == "default":
        return inv_freq
    if kind == "linear":
        return inv_freq / float(rope_scaling["factor"])
    if kind != "llama3":
        raise NotImplementedError(f"rope_scaling type {kind!r} is not implemented (default, linear, llama3 are)")
    factor = float(rope_scaling["factor"])
    lo, hi = float(rope_scaling["low_freq_factor"]), float(rope_scaling["high_freq_factor"])
    old_len = float(rope_scaling["original_max_position_embeddings"])
    wavelen = 2.0 * math.pi / inv_freq
    blend = ((old_len / wavelen - lo) / (hi - lo)).clamp(0.0, 1.0)  # 0: long wavelengths (scaled), 1: short ones (kept)
    scaled = inv_freq / factor
    out = torch.where(wavelen > old_len / lo, scaled, torch.where(wavelen < old_len / hi, inv_freq, (1.0 - blend) * scaled + blend * inv_freq))
    return out.to(torch.float32)


def rope_tables(head_dim: int, max_seq: int, base: float, device, dtype=torch.float16, rope_scaling: Optional[dict] = None):
    """cos/sin [max_seq, head_dim] as LlamaRotaryEmbedding.forward produces them (model.py:343-405): inv_freq in fp32
    (`rope_inv_freq`), freqs = pos * inv_freq, emb = cat(freqs, freqs), cos/sin in fp32, then cast to the activation dtype
    (attention_scaling == 1 for default / linear / llama3)."""
    inv_freq = rope_inv_freq(head_dim, base, rope_scaling, device)
    pos = torch.arange(max_seq, device=device, dtype=torch.float32)
    freqs = torch.outer(pos, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype).contiguous(), emb.sin().to(dtype).contiguous()


def rotate_half(x):
    x1 = x[..., :x.shape[-1] // 2]
    x2 = x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1):
    cos = cos.unsqueeze(unsqueeze_dim)
    sin = sin.unsqueeze(unsqueeze_dim)
    q_embed = (q * cos) + (rotate_half(q) * sin)
    k_embed = (k * cos) + (rotate_half(k) * sin)
    return q_embed, k_embed


def window_mask(n: int, window: Optional[int], device=None) -> Tensor:
    """bool [n, n], True where query row q attends key column kv: causal (kv <= q), and with a window W also kv > q - W -- transformers'
    masking_utils.sliding_window_overlay on top of the causal mask"""
    q = torch.arange(n, device=device)[:, None]
    kv = torch.arange(n, device=device)[None, :]
    m = kv <= q
    return m if window is None else m & (kv > q - int(window))


MASK_TABLE_MAX = 16384  # rows of a cache up to which setup_caches keeps [n, n] mask tables (1 GiB per table at 32768 rows: none above)


FP8_MAX = 448.0  # the largest e4m3 magnitude


def kv_cache_dtype_name(kv_cache_dtype) -> str:
    """None / "fp16" -> "fp16" (the cache in the model's own dtype: the default), "fp8" -> "fp8" (OCP e4m3 codes + a scale per KV head)"""
    name = "fp16" if kv_cache_dtype is None else str(kv_cache_dtype)
    if name not in ("fp16", "fp8"):
        raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}: None, 'fp16' or 'fp8'")
    return name


def fp8_quantize(x16: Tensor, inv: Tensor) -> Tensor:
    """THE write rule of the fp8 cache (include/gq_hip.h), the only rounding the format adds: code = fp8_rne(clamp(float(x16) * inv,
    -448, 448)).  x16 [.., n_kv_head, n, head_dim], inv fp32 [n_kv_head]; returns the codes as uint8."""
    return (x16.float() * inv[:, None, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


class KVCache(nn.Module):
    """k_cache / v_cache [batch][n_kv_head][max_seq][head_dim] in `dtype`.  fp8=True: torch.float8_e4m3fn caches with four fp32
    [n_kv_head] buffers -- k_scale / v_scale (value = code * scale, default 1.0) and their reciprocals k_inv / v_inv, which the host
    fills (`set_scales`: torch.reciprocal; no kernel divides).  `dtype` is then what `update` dequantises to."""

    def __init__(self, max_batch_size, max_seq_length, n_heads, head_dim, dtype=torch.half, device=None, fp8=False):
        super().__init__()
        cache_shape = (max_batch_size, n_heads, max_seq_length, head_dim)
        self.fp8, self.out_dtype = bool(fp8), dtype
        store = torch.float8_e4m3fn if fp8 else dtype
        self.register_buffer('k_cache', torch.zeros(cache_shape, dtype=store, device=device))
        self.register_buffer('v_cache', torch.zeros(cache_shape, dtype=store, device=device))
        if fp8:
            for name in ("k_scale", "v_scale", "k_inv", "v_inv"):
                self.register_buffer(name, torch.ones(n_heads, dtype=torch.float32, device=device))

    def set_scales(self, k_scale, v_scale):
        """new scales IN PLACE (the kernels read them from device memory: a captured graph sees them at its next replay)"""
        assert self.fp8
        self.k_scale.copy_(k_scale)
        self.v_scale.copy_(v_scale)
        self.k_inv.copy_(torch.reciprocal(self.k_scale))
        self.v_inv.copy_(torch.reciprocal(self.v_scale))

    def dequant(self, cache, scale):
        """the read rule: value = float(code) * scale, handed on in the model's dtype"""
        return (cache.float() * scale[:, None, None]).to(self.out_dtype)

    def update(self, input_pos, k_val, v_val):
        assert input_pos.shape[0] == k_val.shape[2]
        if self.fp8:  # stored by the write rule, returned dequantised: the module forward restates what the HIP route computes
            self.k_cache.view(torch.uint8)[:, :, input_pos] = fp8_quantize(k_val, self.k_inv)
            self.v_cache.view(torch.uint8)[:, :, input_pos] = fp8_quantize(v_val, self.v_inv)
            return self.dequant(self.k_cache, self.k_scale), self.dequant(self.v_cache, self.v_scale)
        k_out = self.k_cache
        v_out = self.v_cache
        k_out[:, :, input_pos] = k_val
        v_out[:, :, input_pos] = v_val
        return k_out, v_out


class RMSNorm(nn.Module):

    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def _norm(self, x):
        return x * torch.rsqrt(torch.mean(x * x, dim=-1, keepdim=True) + self.eps)

    def forward(self, x: Tensor) -> Tensor:
        output = self._norm(x.float()).type_as(x)
        return output * self.weight


class Attention(nn.Module):

    def __init__(self, config: ModelArgs, linear_class=nn.Linear, linear_kwargs=None, fuse_linears=True) -> None:
        super().__init__()
        total_head_dim = (config.n_head + 2 * config.n_local_heads) * config.head_dim
        if fuse_linears:
            self.wqkv = linear_class(config.dim, total_head_dim, bias=config.attn_bias, **(linear_kwargs or {}))
        else:
            self.wq = linear_class(config.dim, config.n_head * config.head_dim, bias=config.attn_bias, **(linear_kwargs or {}))
            self.wk = linear_class(config.dim, config.n_local_heads * config.head_dim, bias=config.attn_bias, **(linear_kwargs or {}))
            self.wv = linear_class(config.dim, config.n_local_heads * config.head_dim, bias=config.attn_bias, **(linear_kwargs or {}))
        self.wo = linear_class(config.n_head * config.head_dim, config.dim, bias=False, **(linear_kwargs or {}))
        if config.qk_norm:  # (modeling_qwen3.Qwen3Attention: Qwen3RMSNorm(head_dim) -- RMSNorm.forward has its rounding points)
            self.q_norm = RMSNorm(config.head_dim, eps=config.norm_eps)
            self.k_norm = RMSNorm(config.head_dim, eps=config.norm_eps)
        self.qk_norm = config.qk_norm
        self.kv_cache = None
        self.n_head = config.n_head
        self.head_dim = config.head_dim
        self.n_local_heads = config.n_local_heads
        self.dim = config.dim
        self.config = config
        self.fuse_linears = fuse_linears

    def forward(self, x: Tensor, mask: Tensor, input_pos: Tensor, cos: Tensor, sin: Tensor) -> Tensor:
        bsz, seqlen, _ = x.shape
        kv_size = self.n_local_heads * self.head_dim
        if self.fuse_linears:
            q, k, v = self.wqkv(x).split([self.n_head * self.head_dim, kv_size, kv_size], dim=-1)
        else:
            q, k, v = self.wq(x), self.wk(x), self.wv(x)
        q = q.view(bsz, seqlen, self.n_head, self.head_dim)
        k = k.view(bsz, seqlen, self.n_local_heads, self.head_dim)
        v = v.view(bsz, seqlen, self.n_local_heads, self.head_dim)
        if self.qk_norm:
            q, k = self.q_norm(q), self.k_norm(k)
        q, k, v = map(lambda t: t.transpose(1, 2), (q, k, v))
        q, k = apply_rotary_pos_emb(q, k, cos[input_pos].unsqueeze(0), sin[input_pos].unsqueeze(0))
        if self.kv_cache is not None:
            k, v = self.kv_cache.update(input_pos, k, v)
        k = k.repeat_interleave(self.n_head // self.n_local_heads, dim=1)
        v = v.repeat_interleave(self.n_head // self.n_local_heads, dim=1)
        y = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0)
        y = y.transpose(1, 2).contiguous().view(bsz, seqlen, -1)
        return self.wo(y)


class FeedForward(nn.Module):

    def __init__(self, config: ModelArgs, linear_class=nn.Linear, linear_kwargs=None, fuse_linears=True) -> None:
        super().__init__()
        self.config = config
        self.fuse_linears = fuse_linears
        if fuse_linears:
            self.w1w3 = linear_class(config.dim, config.intermediate_size * 2, bias=False, **(linear_kwargs or {}))
            if hasattr(self.w1w3, "lut"):  # Any-Precision linear: the fused decode step may pair its rows in place
                self.w1w3._register_state_dict_hook(_unpair_on_export)
                self.w1w3._register_load_state_dict_pre_hook(_incoming_is_reference_layout, with_module=True)
        else:
            self.w1 = linear_class(config.dim, config.intermediate_size, bias=False, **(linear_kwargs or {}))
            self.w3 = linear_class(config.dim, config.intermediate_size, bias=False, **(linear_kwargs or {}))
        self.w2 = linear_class(config.intermediate_size, config.dim, bias=False, **(linear_kwargs or {}))
        self.act_fn = F.silu

    def forward(self, x: Tensor) -> Tensor:
        if self.fuse_linears and getattr(self.w1w3, "gq_row_pairs", False):
            # the fused decode step re-ordered this tensor's rows to (gate_0, up_0, gate_1, up_1, ..) in place
            # (`pair_gate_up_rows_`): the module forward (prefill, tests) reads the interleaved output back
            y = self.w1w3(x)
            w1_out, w3_out = y[..., 0::2], y[..., 1::2]
        elif self.fuse_linears:
            # .clone(): the quantized linears return their persistent output buffer by reference
            w1_out, w3_out = self.w1w3(x).split([self.config.intermediate_size, self.config.intermediate_size], dim=-1)
        else:
            w1_out = self.w1(x).clone()
            w3_out = self.w3(x)
        return self.w2(self.act_fn(w1_out) * w3_out)


def _pair_perm(inter: int, device):
    """row order (gate_0, up_0, gate_1, up_1, ..) of a fused [w1; w3] tensor"""
    return torch.stack((torch.arange(inter, device=device), torch.arange(inter, 2 * inter, device=device)), dim=1).reshape(-1)


def pair_gate_up_rows_(m) -> None:
    """Re-order the rows of a fused gate/up Any-Precision linear IN PLACE to interleaved (gate_i, up_i) pairs, the layout
    the GQ_EPI_SILU_PAIRS epilogue consumes (the w1w3 GEMV then writes silu(gate) * up directly).  No second copy of the
    tensor is kept (round 1 held one: +0.94 GB at 8B 2-bit, +3.8 GB at 70B).  The state-dict contract is unchanged:
    `state_dict()` exports the reference layout [w1; w3] (hook below) and `load_state_dict` takes it."""
    if getattr(m, "gq_row_pairs", False):
        return
    perm = _pair_perm(m.out_features // 2, m.qweight.device)
    m.qweight.data = m.qweight.data[:, perm, :].contiguous()
    m.lut.data = m.lut.data[perm].contiguous()
    m.gq_row_pairs = True
    m.gq_realloc_gen = getattr(m, "gq_realloc_gen", 0) + 1  # (new tensors: captured graphs must re-validate, Transformer._alloc_gen)


def _unpair_on_export(module, state_dict, prefix, local_metadata):
    if getattr(module, "gq_row_pairs", False):
        inter = module.out_features // 2
        inv = torch.argsort(_pair_perm(inter, state_dict[prefix + "lut"].device))
        state_dict[prefix + "qweight"] = state_dict[prefix + "qweight"][:, inv, :].contiguous()
        state_dict[prefix + "lut"] = state_dict[prefix + "lut"][inv].contiguous()


def _incoming_is_reference_layout(module, state_dict, prefix, *args, **kwargs):
    # load_state_dict brings [w1; w3]; the native state is rebuilt (and re-paired) lazily.  Only when this module's tensors are
    # actually in the incoming dict: a strict=False load without them leaves the paired rows (and the flag) as they are.
    if prefix + "qweight" in state_dict or prefix + "lut" in state_dict:
        module.gq_row_pairs = False


class TransformerBlock(nn.Module):

    def __init__(self, config: ModelArgs, linear_class=nn.Linear, linear_kwargs=None, fuse_linears=True) -> None:
        super().__init__()
        self.attention = Attention(config, linear_class, linear_kwargs, fuse_linears)
        self.feed_forward = FeedForward(config, linear_class, linear_kwargs, fuse_linears)
        if any(n in config.model_name.lower() for n in ("llama", "mistral", "qwen3", "qwen2")):  # (one block layout: pre-norm, gated MLP)
            self.input_layernorm = RMSNorm(config.dim, config.norm_eps)
            self.post_attention_layernorm = RMSNorm(config.dim, config.norm_eps)
        else:
            raise NotImplementedError

    def forward(self, x: Tensor, input_pos: Tensor, mask: Tensor, cos: Tensor, sin: Tensor) -> Tensor:
        h = x + self.attention(self.input_layernorm(x), mask, input_pos, cos, sin)
        out = self.feed_forward(self.post_attention_layernorm(h))
        return h + out


class Transformer(nn.Module):

    def __init__(self, dtype, config: ModelArgs, linear_class=nn.Linear, linear_kwargs=None, halve_layers=False,
                 fuse_linears=True) -> None:
        super().__init__()
        self.config = config
        self.dtype = dtype
        if halve_layers:
            config.n_layer = config.n_layer // 2
            if config.layer_windows is not None:
                config.layer_windows = config.layer_windows[:config.n_layer]
        self.tok_embeddings = nn.Embedding(config.vocab_size, config.dim)
        self.layers = nn.ModuleList(
            TransformerBlock(config, linear_class, linear_kwargs, fuse_linears) for _ in range(config.n_layer))
        self.norm = RMSNorm(config.dim, eps=config.norm_eps)
        self.output = nn.Linear(config.dim, config.vocab_size, bias=False)
        self.max_batch_size = -1
        self.max_seq_length = -1
        self.kv_cache_dtype = "fp16"
        self.cache_initialized = False
        self.fuse_linears = fuse_linears
        self._native = None
        self.lm_head_dtype = "fp16"  # set_lm_head_dtype
        self._head_q8 = None         # (q int8 [V, D], scale fp32 [V], the output.weight they were made from): plain attributes, not buffers
        # new weights (copied in place or assigned): the native step's buffers / launch plans / row pairing are rebuilt lazily
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module._weights_changed())

    def _reset_native(self):
        self._native = None
        self._native_kind_cache = None
        self._alloc_gen = getattr(self, "_alloc_gen", 0) + 1  # captured graphs re-validate their pointers (generate.DecodeGraph.step)

    def _weights_changed(self):
        self._head_q8 = None  # (the int8 copy of the head follows output.weight; a cache that grows does not come through here)
        self._reset_native()

    def _apply(self, fn, *a, **k):
        # .to() / .half() / .cuda() move or re-allocate every tensor a captured decode graph points at
        r = super()._apply(fn, *a, **k)
        self._weights_changed()
        return r

    def set_lm_head_dtype(self, name) -> None:
        """The head of the fused decode step: None / "fp16" (the default: gq_dense_gemv_f16 over `output.weight`, as the reference) or
        "int8" (gq_dense_gemv_i8 over a weight-only int8 copy with one fp32 scale per row, head_q8.quantize_rows_int8).  "int8"
        quantises `output.weight` once, on its device, into tensors that are no part of the state_dict, and keeps `output.weight`: the
        prompt pass, `score()` and the module forward read the fp16 head, a tied embedding is untouched.  Cost: N*K + 4N bytes NEXT TO
        the fp16 head (0.53 GB for the 128256 x 4096 head of Llama-3.1-8B).  The copy is rebuilt when `output.weight` is another tensor
        or has been written (load_state_dict, .to() / .half(), an in-place write), not when the caches grow.  ValueError on a CPU model
        or a head that is not fp16."""
        from .head_q8 import lm_head_dtype_name
        name = lm_head_dtype_name(name)
        if name == "int8":
            self._head_q8_check()
        self.lm_head_dtype = name
        self._head_q8 = None
        if name == "int8":
            self.head_q8()
        self._reset_native()

    def _head_q8_check(self):
        w = self.output.weight
        if not w.is_cuda:
            raise ValueError("lm_head_dtype='int8': the int8 head is served by the fused HIP decode step only, and the model is on the CPU")
        if w.dtype != torch.float16:
            raise ValueError(f"lm_head_dtype='int8': output.weight is {w.dtype}, not fp16")

    def head_q8(self):
        """(q int8 [V, D], scale fp32 [V]) of an int8-head model, made again where `output.weight` changed since they were made"""
        from .head_q8 import quantize_rows_int8
        assert self.lm_head_dtype == "int8", "head_q8: the model's head is fp16 (set_lm_head_dtype('int8'))"
        w = self.output.weight
        made = self._head_q8
        key = (w.data_ptr(), 0 if w.is_inference() else w._version)  # (an inference tensor counts no writes: it cannot be written)
        if made is None or made[2] != key:
            self._head_q8_check()
            q, scale = quantize_rows_int8(w.detach())
            self._head_q8 = made = (q, scale, key)
            self._alloc_gen = getattr(self, "_alloc_gen", 0) + 1  # (new tensors: captured graphs re-validate their pointers)
        return made[0], made[1]

    @classmethod
    def from_name(cls, dtype, name: str, linear_class=nn.Linear, linear_kwargs=None, halve_layers=False,
                  fuse_linears=True) -> "Transformer":
        return cls(dtype, ModelArgs.from_name(name), linear_class=linear_class, linear_kwargs=linear_kwargs,
                   halve_layers=halve_layers, fuse_linears=fuse_linears)

    def kv8_unserved(self) -> Optional[str]:
        """why the fused HIP route cannot serve this model with an fp8 KV cache (None: it can).  Host logic, no device needed."""
        from .APLinear import APLinear
        if not self.fuse_linears:
            return "the model is not a fused-linear Any-Precision model"
        if self.config.head_dim not in (64, 128):
            return f"head_dim {self.config.head_dim} (the fp8 launches serve 64 and 128)"
        if not all(isinstance(m, APLinear) for b in self.layers for m in (b.attention.wqkv, b.attention.wo, b.feed_forward.w1w3, b.feed_forward.w2)):
            return "the linears are not Any-Precision linears"
        if self.output.weight.dtype != torch.float16:
            return "the model is not fp16"
        return None

    def setup_caches(self, max_batch_size, max_seq_length, kv_cache_dtype=None):
        """kv_cache_dtype: None / "fp16" (the default: caches in the model's dtype) or "fp8" (e4m3 codes, a scale per layer and KV head,
        `set_kv_scales`; served by the fused Any-Precision route and the module forward).  A change of the dtype re-allocates the caches
        even when their size suffices."""
        kv = kv_cache_dtype_name(kv_cache_dtype)
        if self.max_seq_length >= max_seq_length and self.max_batch_size >= max_batch_size and kv == self.kv_cache_dtype:
            return
        if kv == "fp8" and not self.fuse_linears and type(self.layers[0].attention.wq).__name__ == "QuantizedLinear":
            raise NotImplementedError("fp8 KV cache: QTIP models keep the fp16 cache (gq_attn_decode_qtip has no fp8 form)")
        head_dim = self.config.head_dim
        max_seq_length = find_multiple(max_seq_length, 8)
        self.max_seq_length = max_seq_length
        self.max_batch_size = max_batch_size
        dtype = self.output.weight.dtype
        device = self.output.weight.device
        for b in self.layers:
            b.attention.kv_cache = KVCache(max_batch_size, max_seq_length, self.config.n_local_heads, head_dim, dtype, device, fp8=(kv == "fp8"))
        self.kv_cache_dtype = kv
        # the [n, n] tables only for a cache of at most MASK_TABLE_MAX rows (tests and pipeline.py index them); above it every consumer
        # builds the rows it needs from the positions (mask_rows: the same bits)
        lw = self.config.layer_windows or ()
        self._window_set = sorted({w for w in lw if w is not None and w < self.max_seq_length})
        if self.max_seq_length <= MASK_TABLE_MAX:
            self.causal_mask = torch.tril(torch.ones(self.max_seq_length, self.max_seq_length, dtype=torch.bool, device=device))
            # one mask per distinct window that is shorter than the cache (a window the cache never outgrows is the causal mask)
            self.window_masks = {w: window_mask(self.max_seq_length, w, device) for w in self._window_set}
        else:
            self.causal_mask, self.window_masks = None, None
        self.rope_cos, self.rope_sin = rope_tables(head_dim, max_seq_length, self.config.rope_base, device, dtype,
                                                   rope_scaling=self.config.rope_scaling)
        self.cache_initialized = True
        self._reset_native()

    def set_kv_scales(self, k: Tensor, v: Tensor) -> None:
        """the scales of an fp8 cache, fp32 [n_layer][n_kv_head] each (value = code * scale; default 1.0), every entry finite and > 0.
        Written in place into the caches' buffers, reciprocals with them: no re-allocation, a captured decode graph needs no re-capture.
        Rows already in the caches keep their codes: set the scales before the prompt."""
        if not (self.cache_initialized and self.kv_cache_dtype == "fp8"):
            raise ValueError("set_kv_scales: the caches are not fp8 (setup_caches(.., kv_cache_dtype='fp8') first)")
        shape = (len(self.layers), self.config.n_local_heads)
        ts = []
        for name, t in (("k", k), ("v", v)):
            t = torch.as_tensor(t, dtype=torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"set_kv_scales: {name} has shape {tuple(t.shape)}, expected [n_layer][n_kv_head] = {shape}")
            if not bool((torch.isfinite(t) & (t > 0)).all()):
                raise ValueError(f"set_kv_scales: every entry of {name} must be finite and > 0")
            ts.append(t)
        for i, b in enumerate(self.layers):
            b.attention.kv_cache.set_scales(ts[0][i], ts[1][i])

    def forward(self, idx: Tensor, input_pos: Optional[Tensor] = None) -> Tensor:
        assert self.cache_initialized, "Caches must be initialized first"
        if self.causal_mask is not None:
            mask = self.causal_mask[None, None, input_pos]
            wmask = {w: wm[None, None, input_pos] for w, wm in self.window_masks.items()}  # (empty for a model without windows)
        else:  # (a cache beyond MASK_TABLE_MAX rows keeps no tables)
            mask = mask_rows(input_pos, self.max_seq_length)[None, None]
            wmask = {w: mask_rows(input_pos, self.max_seq_length, w)[None, None] for w in self._window_set}
        lw = self.config.layer_windows or (None,) * len(self.layers)
        x = self.tok_embeddings(idx)
        for layer, w in zip(self.layers, lw):
            x = layer(x, input_pos, wmask.get(w, mask), self.rope_cos, self.rope_sin)
        x = self.norm(x)
        return self.output(x)

    # ------------------------------------------------------------------------------------------ fused HIP decode step
    # (guidedquant_amd/native_step.py: the buffers, launch plans and launches; here its surface on the model)
    def native_ready(self) -> bool:
        return self._native_kind() is not None

    def _native_kind(self):
        """'ap': fused-linear Any-Precision model (<= 8 bit) -> gq_anyprec_gemv_fused chain; 'qtip': unfused QTIP model
        with power-of-two widths -> gq_qtip_linear_in / _out chain; None: the module-by-module forward."""
        from .APLinear import APLinear
        if not (self.cache_initialized and self.output.weight.is_cuda):
            return None
        if self.output.weight.dtype != torch.float16 or self.max_batch_size < 1:
            return None
        kind = getattr(self, "_native_kind_cache", None)
        if kind is not None:
            return kind or None
        kind = ""
        if self.config.qk_norm and (self.config.head_dim not in (64, 128) or not self.fuse_linears):
            pass  # (QK-norm is served by gq_attn_decode_split_qknorm, head_dim 64 / 128, fused Any-Precision models: else the module forward)
        elif self.fuse_linears:
            # (a bias only where the block layout has one -- wqkv of an attn_bias model -- and the attention launch that adds it serves the
            # head_dim: gq_attn_decode_split_bias, 64 / 128; a bias anywhere else has no fused form)
            # (and not next to QK-norm: the bias form and the norm form of the launch do not combine)
            qkv_bias_ok = self.config.attn_bias and not self.config.qk_norm and self.config.head_dim in (64, 128)
            if all(isinstance(m, APLinear) and (m.bias is None or (qkv_bias_ok and m is b.attention.wqkv)) and m.bitwidth <= 8
                   and m.in_features % 128 == 0
                   for b in self.layers for m in (b.attention.wqkv, b.attention.wo, b.feed_forward.w1w3, b.feed_forward.w2)):
                kind = "ap"
        elif native_step.native_qtip() and self.config.layer_windows is None:  # (no window form of gq_attn_decode_qtip)
            from .qtip import QuantizedLinear

            p2 = lambda n: n > 0 and (n & (n - 1)) == 0  # noqa: E731

            def ok(m):
                # widths: power of two (fused transform), or Kf * 2^p with the caller's Hadamard factor table loaded
                # (gq_qtip_transform; e.g. 11008 = 172 * 64, 5120 = 20 * 256)
                def side(nf, K, had):
                    return p2(nf) if K == 1 else (had is not None and p2(nf // K) and nf // K >= 64 and nf <= 32768)
                return (isinstance(m, QuantizedLinear) and m.bias is None and m.has_kernel and int(m.rcp.item()) == 0
                        and side(m.in_features, m.K_left, m.had_left) and side(m.out_features, m.K_right, m.had_right)
                        and 32 <= m.in_features and (m.in_features <= 16384 or m.K_left != 1) and m.out_features <= 32768)
            if self.config.head_dim in (64, 128) and all(
                    ok(m) for b in self.layers for m in (b.attention.wq, b.attention.wk, b.attention.wv, b.attention.wo,
                                                         b.feed_forward.w1, b.feed_forward.w3, b.feed_forward.w2)):
                kind = "qtip"
        self._native_kind_cache = kind
        return kind or None

    def _native_state(self):
        """buffers and launch plans of the step (native_step.ApStep / QtipStep), built on first use; subscriptable by field name"""
        if self._native is None:
            self._native = (native_step.QtipStep if self._native_kind() == "qtip" else native_step.ApStep)(self)
        return self._native

    def native_embed(self, tok: Tensor, x: Tensor, ssq: Optional[Tensor] = None):
        """x = tok_embeddings[tok]; with `ssq` (the hand-over slots of _native_state) also the statistics of x for layer 0's RMSNorm"""
        native_step.embed(self, tok, x, ssq)

    def _handover_plan(self, blk):
        """which RMSNorm edges of a layer hand their statistics over (native_step.handover_plan; GQ_SSQ_HANDOVER, off by default)"""
        return native_step.handover_plan(self, blk)

    def native_layers(self, x: Tensor, pos: Tensor, l0: int, l1: int, slot: int = 0, ssq_ready: bool = False):
        """layers [l0, l1) of one decode step, in place on the hidden state `x` (fp16 [dim]); `slot` = batch index of
        the KV caches to use (layer-pipelined decode keeps one sequence per slot).  ssq_ready: the hand-over slots hold the
        statistics of `x` (native_embed(..., ssq) ran on it)."""
        self._native_state().layers(x, pos, l0, l1, slot, ssq_ready)

    def native_head(self, x: Tensor) -> Tensor:
        return self._native_state().head(x)

    # ------------------------------------------------------------------------------------------------ prompt pass
    # (guidedquant_amd/native_prompt.py: the chunk loop, one piece, the heads; here its surface on the model)
    def prefill_ready(self, idx: Tensor) -> bool:
        """the HIP prompt pass serves what the native decode step serves (fused Any-Precision models, unfused QTIP models):
        fp16, batch 1, on the GPU"""
        return native_prompt.ready(self, idx)

    def prefill_native(self, idx: Tensor, input_pos: Tensor, start: int = 0, last_only: bool = True, chunk: Optional[int] = None) -> Tensor:
        """The prompt pass (`Transformer.forward` with seq_len > 1, inference/model.py:206-266 semantics) with the element-wise
        steps between the linears as ONE HIP launch each (csrc/prefill.hip: RMSNorm rows, RoPE + KV-cache write, silu * up)
        instead of ~45 eager tensor ops per layer, the linears through `APLinear.forward` (fused prefill GEMM / split K /
        the reference's two steps by size) or, for QTIP models, `QuantizedLinear.forward` (the trellis-decode GEMM), attention
        over the keys [0, start + S) only instead of the whole cache.
        `input_pos` must be arange(start, start + S) (what generate() passes; `start` is the host copy of its first element).
        Same fp16 rounding points as the module forward: logits agree up to the summation order of the fp32 sums.
        last_only: logits of the last prompt token only, [1, 1, V] -- all generate() samples from -- else [1, S, V].
        chunk (None: GQ_PREFILL_CHUNK, default 4096): a prompt of more than `chunk` tokens goes through in pieces of `chunk` tokens
        (`prefill_chunks`: chunks outer, layers inner, over the same caches; a tail of one token included), so the intermediates are
        sized by the chunk, not by the prompt; with last_only only the last piece runs the head.
        Attention follows GQ_PREFILL_ATTN: "auto" (default) -- the HIP kernel gq_attn_prefill (csrc/prefill_attn.hip) inside a chunked
        pass where gq_attn_prefill_supported, torch SDPA everywhere else (a prompt of at most `chunk` tokens launches what it always
        did); "1" -- the kernel wherever it is supported; "0" -- never.  `last_prefill_plan` records what the pass did:
        dict(chunks=[(start, S), ..], attn=["hip" | "sdpa" per layer])."""
        return native_prompt.prompt_pass(self, idx, input_pos, start, last_only, chunk)

    SCORE_HEAD_ROWS = 512  # rows per block of the torch scoring head: its fp16 + fp32 logits are bounded by 512 x V x 6 bytes
    # what GQ_SCORE_HEAD=auto takes where the kernel serves the shape: the kernel -- no slower than the torch head at both measured sizes
    # (8B geometry: 3.2 against 3.6 ms at 2048 rows, 6.4 against 7.1 ms at 4096; profiles/score_head.json)
    SCORE_HEAD_AUTO = "1"

    def _score_head(self, x: Tensor, targets: Tensor, kernel: bool):
        """the scoring head on the residual rows x fp16 [n, D] and targets int32 [n] (negative: ignored, logprob 0): (logprob fp32 [n],
        top1 [n]).  Both forms read the fp16 rows norm(x) the logits head feeds to `self.output`: the kernel gq_head_nll
        (csrc/head_nll.hip; no logits in memory), or output -> float -> log_softmax -> gather / argmax in blocks of SCORE_HEAD_ROWS rows."""
        return native_prompt.score_head(self, x, targets, kernel)

    def score_native(self, idx: Tensor, chunk: Optional[int] = None):
        """Log-probabilities of a token sequence on the HIP prompt pass: (logprob fp32 [S - 1], greedy bool [S - 1]) with
        logprob[i] = log p(idx[i + 1] | idx[:i + 1]) and greedy[i] = (the most probable next token == idx[i + 1]) -- what the module tree's
        `labels=` loss and lm-eval's loglikelihood are made of.  The pass is `prefill_native`'s from position 0 (the same pieces, caches,
        GQ_PREFILL_CHUNK and GQ_PREFILL_ATTN; everything `prefill_ready` serves, the fp8 cache included) with the scoring head on every
        piece, so no [S, V] logits exist.  GQ_SCORE_HEAD: "1" the kernel gq_head_nll, "0" the torch head in blocks of 512 rows, "auto"
        (default) SCORE_HEAD_AUTO where the kernel serves the shape (dim % 64 == 0, fp16) and the torch head elsewhere.
        `last_prefill_plan["head"]` records it ("hip-nll" | "torch").  The caches hold the sequence afterwards, as after a prompt."""
        return native_prompt.score(self, idx, chunk)

    def score_packed_native(self, seqs, rows: Optional[Tensor] = None):
        """Log-probabilities of SEVERAL token sequences in one HIP prompt pass (varlen attention): the sequences are laid end to end as
        one run of S rows from cache row 0 and go through every layer as ONE piece, so the weights are read once per pack.  Row i is
        rotated by its position inside its own sequence (gq_rope_cache_rows_packed) and attends only rows of its own sequence, causally
        and within the layer's window (gq_attn_prefill_packed; under GQ_PREFILL_ATTN=0 or an unserved geometry SDPA with the
        block-diagonal mask).  `rows` (bool [S]): only these rows reach the final norm and the scoring head.  Returns (logprob fp32 [k],
        hit bool [k]) over the head's rows in packed order (native_prompt.score_packed).  fp16 caches only; the caches grow to S rows
        where they are smaller and hold the pack afterwards.  `last_prefill_plan` records chunks=[(0, S)], attn "hip-packed" |
        "sdpa-packed" per layer, the head and packed=dict(sequences, rows, head_rows)."""
        return native_prompt.score_packed(self, seqs, rows)

    def decode_native(self, tok: Tensor, pos: Tensor) -> Tensor:
        """One bs=1 decode step.  tok, pos: int32 device tensors with one element.  Returns logits fp16 [1,1,V]
        (a persistent buffer, like the quantized linears' outputs).  Enqueues on the current stream only."""
        assert tok.dtype == torch.int32 and pos.dtype == torch.int32 and tok.is_cuda and pos.is_cuda
        with torch.cuda.device(self.output.weight.device):  # (launches go to the model's device's current stream)
            st = self._native_state()
            x = st["x"]
            ho0 = self._native_kind() == "ap" and self._handover_plan(self.layers[0])["qkv_in"]
            self.native_embed(tok, x, st["ssq"] if ho0 else None)
            self.native_layers(x, pos, 0, len(self.layers), ssq_ready=bool(ho0))
            return self.native_head(x)
