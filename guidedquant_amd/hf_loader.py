"""Loader for HF-layout GuidedQuant / Any-Precision checkpoints: a directory with
`config.json` (a Llama, Mistral, Qwen2 or Qwen3 config plus the `anyprec` section, any_precision/modules/AnyPrecisionForCausalLM.py:43-47) and the
weights as `pytorch_model.bin` or (sharded) safetensors with the HF keys `model.layers.{i}.self_attn.q_proj.{qweight,lut{b}}`
(any_precision/quantization/pack.py:112-123) -> the fused gpt-fast `Transformer` of this package, ready for the HIP
decode path.  Equivalent to running inference/sqllm_llama_convert_fuse.py and then inference/generate.py::load_model,
without the intermediate file and without the "Llama-2-*" directory-name restriction (any layer count / GQA geometry).
Host code only; plain torch.load / safetensors and manual device placement (no accelerate dispatch)."""
import glob
import json
import os

import torch

from .APLinear import APLinear
from .convert import convert_anyprec_fuse
from .model import ModelArgs, Transformer


def _no_sliding_window(cfg: dict, what: str):
    """for a caller that attends over the whole cache (model_args_from_hf_config without sliding_window=True): a checkpoint whose layers use
    a sliding window shorter than its context is declined"""
    lt = cfg.get("layer_types")
    if lt and any(t != "full_attention" for t in lt):
        raise NotImplementedError(f"{what}: layer_types {sorted(set(lt))} (only full_attention layers have a fused decode form)")
    if what == "qwen2" and "use_sliding_window" not in cfg and not lt:
        # (every Qwen2 config.json transformers has written carries `use_sliding_window`, and newer ones `layer_types` as well: a dict
        # that names the model type and states neither is not such a file, and whether its layers attend over the whole cache is a guess)
        raise NotImplementedError("qwen2: the config states neither use_sliding_window nor layer_types (a Qwen2 config.json does; the fused "
                                  "decode form attends over the whole cache and does not guess)")
    if what in ("qwen2", "qwen3") and cfg.get("use_sliding_window"):
        raise NotImplementedError(f"{what}: use_sliding_window (sliding-window attention has no fused decode form)")
    sw = cfg.get("sliding_window")
    if what == "mistral" and sw is not None and int(sw) < int(cfg.get("max_position_embeddings", 8192)):
        raise NotImplementedError(f"mistral: sliding_window {sw} < max_position_embeddings (sliding-window attention has no fused decode form)")


def _layer_windows(cfg: dict, what: str):
    """the window of every layer (None: the whole context), as transformers resolves it: from `layer_types` where the config has them
    (full_attention / sliding_attention; anything else -- chunked_attention, .. -- has no fused form), else Mistral: every layer, else
    Qwen2 / Qwen3 with use_sliding_window: the layers i >= max_window_layers.  W = `sliding_window`; a window the context never outgrows
    (W >= max_position_embeddings) is no window."""
    n = int(cfg["num_hidden_layers"])
    lt, sw = cfg.get("layer_types"), cfg.get("sliding_window")
    if lt:
        other = sorted(set(lt) - {"full_attention", "sliding_attention"})
        if other:
            raise NotImplementedError(f"{what}: layer_types {other} (full_attention and sliding_attention layers have a fused decode form)")
        if len(lt) != n:
            raise ValueError(f"{what}: {len(lt)} layer_types for {n} layers")
        sliding = [t == "sliding_attention" for t in lt]
    elif what == "mistral":
        sliding = [sw is not None] * n
    elif what in ("qwen2", "qwen3") and cfg.get("use_sliding_window"):
        first = int(cfg.get("max_window_layers", n))
        sliding = [i >= first for i in range(n)]
    else:
        sliding = [False] * n
    if not any(sliding):
        return None
    if sw is None:
        raise ValueError(f"{what}: sliding-window layers without a sliding_window")
    if int(sw) < 1:
        raise ValueError(f"{what}: sliding_window {sw}")
    if int(sw) >= int(cfg.get("max_position_embeddings", 8192)):
        return None
    return tuple(int(sw) if s else None for s in sliding)


def model_args_from_hf_config(cfg: dict, sliding_window: bool = False) -> ModelArgs:
    """HF `config.json` -> ModelArgs (inference/model.py:27-51 field meanings), by `model_type`:
      llama (or no model_type)  the Llama block;
      mistral                   the same block, head_dim from the config when it has one; only without a sliding window that bites;
      qwen2                     (Qwen2 / Qwen2.5) the same block with a bias on q_proj / k_proj / v_proj (attn_bias); head_dim from the config
                                when it has one, else hidden_size / num_attention_heads; dense full-attention layers only, and the
                                config must say so (`use_sliding_window` or `layer_types`, as every Qwen2 config.json does);
      qwen3                     head_dim of its own and the per-head q / k RMSNorm (qk_norm); dense full-attention layers only, no
                                attention_bias.
    sliding_window=True: a config with sliding-window layers is not declined but resolved to ModelArgs.layer_windows (`_layer_windows`) --
    what the loaders of this package pass, whose decode step and prompt pass serve a per-layer window; the default keeps declining for a
    caller that attends over the whole cache itself.
    Anything else (gemma3*, phi*, opt, MoE models, ..) raises NotImplementedError: the fused decode
    model knows these block layouts and no other, and a layout it does not know must not be decoded as if it were Llama's."""
    mt = str(cfg.get("model_type") or "llama").lower()
    if mt not in ("llama", "mistral", "qwen2", "qwen3"):
        raise NotImplementedError(f"model_type {mt!r} has no fused decode form (llama, mistral, qwen2 and qwen3 dense have)")
    name = os.path.basename(str(cfg.get("_name_or_path") or mt).rstrip("/")) or mt
    if mt not in name.lower():  # (the block layout is the model type's whatever the checkpoint directory is called)
        name = mt + "-" + name
    extra = {}
    if mt != "llama":
        if sliding_window:
            if mt == "qwen2" and "use_sliding_window" not in cfg and not cfg.get("layer_types"):
                _no_sliding_window(cfg, mt)  # (a dict that states neither is no Qwen2 config.json: raises)
            lw = _layer_windows(cfg, mt)
            if lw is not None:
                extra["layer_windows"] = lw
        else:
            _no_sliding_window(cfg, mt)
        if cfg.get("head_dim"):
            extra["head_dim"] = int(cfg["head_dim"])
    if mt == "qwen2":  # (modeling_qwen2.Qwen2Attention: q_proj / k_proj / v_proj with bias=True, o_proj and the MLP without)
        extra["attn_bias"] = True
    if mt == "qwen3":
        if cfg.get("attention_bias"):
            raise NotImplementedError("qwen3: attention_bias (the fused decode step has no form with both the per-head norm and a bias)")
        extra["qk_norm"] = True
    rope_theta, rope_scaling = cfg.get("rope_theta"), cfg.get("rope_scaling")
    rp = cfg.get("rope_parameters")  # (newer transformers keep base and scaling together)
    if isinstance(rp, dict):
        rope_theta = rp.get("rope_theta", rope_theta) if rope_theta is None else rope_theta
        if rope_scaling is None and rp.get("rope_type", "default") != "default":
            rope_scaling = {k: v for k, v in rp.items() if k != "rope_theta"}
    return ModelArgs(block_size=int(cfg.get("max_position_embeddings", 8192)), vocab_size=int(cfg["vocab_size"]),
                     n_layer=int(cfg["num_hidden_layers"]), n_head=int(cfg["num_attention_heads"]), dim=int(cfg["hidden_size"]),
                     intermediate_size=int(cfg["intermediate_size"]),
                     n_local_heads=int(cfg.get("num_key_value_heads") or cfg["num_attention_heads"]),
                     rope_base=float(10000.0 if rope_theta is None else rope_theta), norm_eps=float(cfg.get("rms_norm_eps", 1e-5)),
                     rope_scaling=rope_scaling, model_name=os.path.basename(str(name)), **extra)


def read_hf_state_dict(path: str) -> dict:
    """pytorch_model.bin, model.safetensors or sharded model-*-of-*.safetensors under `path`."""
    p = os.path.join(path, "pytorch_model.bin")
    if os.path.exists(p):
        return torch.load(p, map_location="cpu", weights_only=True)
    files = sorted(glob.glob(os.path.join(path, "*.safetensors")))
    if not files:
        raise FileNotFoundError(f"no pytorch_model.bin / *.safetensors under {path}")
    from safetensors.torch import load_file
    sd = {}
    for f in files:
        sd.update(load_file(f))
    return sd


def supported_precisions(cfg: dict):
    ap = cfg.get("anyprec")
    if not ap:
        raise ValueError("config.json has no 'anyprec' section (not an Any-Precision checkpoint)")
    return list(range(int(ap["seed_precision"]), int(ap["parent_precision"]) + 1))


def load_anyprec_hf(path: str, bitwidth: int = None, device="cuda", dtype=torch.float16) -> Transformer:
    """Build the fused decode model from an HF-layout Any-Precision checkpoint directory at `bitwidth`
    (default: the seed precision, the only one GuidedQuant checkpoints carry, scripts/run_lnq.sh)."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    bits = supported_precisions(cfg)
    if bitwidth is None:
        bitwidth = bits[0]
    if bitwidth not in bits:
        raise ValueError(f"bitwidth {bitwidth} not in the checkpoint's precisions {bits}")
    return anyprec_state_dict_to_transformer(read_hf_state_dict(path), cfg, bitwidth, device, dtype)


def anyprec_state_dict_to_transformer(sd: dict, cfg: dict, bitwidth: int, device="cuda", dtype=torch.float16) -> Transformer:
    """HF-keyed Any-Precision tensors (host or device) + the config dict -> the fused decode model at `bitwidth`"""
    args = model_args_from_hf_config(cfg, sliding_window=True)
    sd = {k: v for k, v in sd.items() if "rotary_emb" not in k}
    if "lm_head.weight" not in sd and cfg.get("tie_word_embeddings", False):
        sd["lm_head.weight"] = sd["model.embed_tokens.weight"]  # tied embeddings (Llama-3.2-1B)
    fused = convert_anyprec_fuse(sd, bitwidth, n_layer=args.n_layer)
    on_dev = all(v.device.type != "cpu" for v in fused.values())
    model = Transformer(dtype, args, linear_class=APLinear, linear_kwargs=dict(bitwidth=bitwidth, device=device if on_dev else "cpu"),
                        fuse_linears=True)
    if on_dev:
        model = model.to(device=device, dtype=dtype)
    model.load_state_dict(fused, strict=True)
    return model.to(device=device, dtype=dtype).eval()
