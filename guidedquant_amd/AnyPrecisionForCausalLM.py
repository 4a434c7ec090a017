"""AnyPrecisionForCausalLM -- the HF-path entry of the reference (any_precision/modules/AnyPrecisionForCausalLM.py:28-210) on
MI355X: an HF causal LM whose decoder linears are `AnyPrecisionLinear` modules (multi-precision parent tensor + one LUT per
precision), with `from_quantized(path, precisions=...)`, `forward(..., precision=b)`, `generate(..., precision=b)`,
`set_precision`, `prune_precisions` -- the harness the reference's only published number (130 tok/s, README.md:95-97,
inference_example.py:34-77) runs on.

Same public surface; the construction is this package's own:
  * the skeleton comes from `AutoModelForCausalLM.from_config` on the meta device; which modules to swap is read from the
    checkpoint's `config.anyprec["arch_config"]` (`model_name`, `layers_name`, `module_names`, pack.py:190-195) -- or, when a
    checkpoint lacks it, every nn.Linear inside the decoder layers -- instead of the reference's analyzer package;
  * weights are read with plain torch / safetensors (hf_loader.read_hf_state_dict) and placed on ONE device: one process
    per GPU is this framework's model (a 70B 2-bit model is 19 GB of a 288 GB HBM), there is no accelerate `device_map`;
  * a rows == 1 call runs the HIP LUT-GEMV (plugin::anyprec_gemv), more rows the dequant + matmul branch, host tensors the
    CPU twins (AnyPrecisionLinear.py).
`native_decoder(bitwidth)` additionally returns the fused gpt-fast `Transformer` of the same checkpoint (hf_loader), whose
decode step is the 5-launches-per-layer hipGraph path bench.py measures.
"""
import gc
import json
import os
import weakref
from typing import List, Optional

import torch
import torch.nn as nn

from .AnyPrecisionLinear import AnyPrecisionLinear
from .hf_loader import read_hf_state_dict


def replace_module_by_name(layer, module_name, new_module):
    levels = module_name.split('.')
    module = layer
    for level in levels[:-1]:
        module = getattr(module, level) if not level.isdigit() else module[int(level)]
    setattr(module, levels[-1], new_module)


def _get_by_path(root, dotted):
    for name in [p for p in dotted.split('.') if p]:
        root = getattr(root, name) if not name.isdigit() else root[int(name)]
    return root


_LOGPROBS_OUTPUT = None


def GenerateLogprobsOutput(**fields):
    """what `generate(output_logprobs=True)` returns: a transformers ModelOutput with `sequences` [1, T + new], `logprobs` and
    `sampled_logprobs` (fp32 [1, new]) and, with top_logprobs=n, `top_logprobs_ids` (int64 [1, new, n]) and `top_logprobs` (fp32 [1, new, n]; both
    None without it).  (The class is made on first use: this module imports transformers lazily.)"""
    global _LOGPROBS_OUTPUT
    if _LOGPROBS_OUTPUT is None:
        import dataclasses
        from transformers.utils import ModelOutput
        _LOGPROBS_OUTPUT = dataclasses.dataclass(type("GenerateLogprobsOutput", (ModelOutput, ), {
            "__annotations__": {"sequences": Optional[torch.Tensor], "logprobs": Optional[torch.Tensor], "sampled_logprobs": Optional[torch.Tensor],
                                "top_logprobs_ids": Optional[torch.Tensor], "top_logprobs": Optional[torch.Tensor]},
            "sequences": None, "logprobs": None, "sampled_logprobs": None, "top_logprobs_ids": None, "top_logprobs": None, "__module__": __name__}))
    return _LOGPROBS_OUTPUT(**fields)


class _WeakRestore:
    """`wrapper._restore_module_tree()` through a weak reference (a state_dict pre-hook of the inner model / the `_gq_restore` of a
    released linear): no reference cycle through the wrapper"""
    __slots__ = ("ref", )

    def __init__(self, wrapper):
        self.ref = weakref.ref(wrapper)

    def __call__(self, *args, **kwargs):
        w = self.ref()
        if w is not None:
            w._restore_module_tree()


class _CapturedStep:
    """State of route 2 (`generate(capture=True)`): the StaticCache, the device words the captured step reads and writes, and the
    hipGraph of one token step of the HF module tree.  A plain object -- no closure over its own state, so no reference cycle owns the
    graph -- with an explicit `close()`: the owner (`AnyPrecisionForCausalLM._evict`) destroys the graph when it drops the entry."""
    __slots__ = ("model", "sampler", "cache", "tok64", "tok", "pos", "nxt", "logits", "graph")

    def __init__(self, model, config, dev, total, temperature, top_k, seed, top_p=1.0, repetition_penalty=1.0, suppress_tokens=()):
        from transformers import StaticCache
        from .fused_sampler import FusedSampler
        self.model = model
        self.cache = StaticCache(config=config, max_cache_len=total)
        # (the fused sampler and its state: counter, workspace, ban, the sequence store and -- with a penalty or a suppress list -- the sets)
        self.sampler = FusedSampler(config.vocab_size, dev, top_k, top_p, temperature, seed, seq_capacity=total + 1,
                                    repetition_penalty=repetition_penalty, suppress_tokens=suppress_tokens)
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
        self.tok64 = z((1, 1), torch.long)
        self.tok, self.pos, self.nxt = z((1, ), torch.int32), z((1, ), torch.int32), z((1, ), torch.int32)
        self.logits = z(int(config.vocab_size), torch.float16)
        self.graph = None

    def step(self):
        # (positions come from the cache itself: StaticLayer.cumulative_length is a device word the layer advances in place)
        out = self.model(input_ids=self.tok64, past_key_values=self.cache, use_cache=True)
        self.logits.copy_(out.logits.view(-1))
        self.sampler.launch(self.logits, self.tok, self.pos, self.nxt)
        self.tok64.copy_(self.tok.view(1, 1))

    def _set_cache_length(self, n):
        for layer in self.cache.layers:
            if torch.is_tensor(getattr(layer, "cumulative_length", None)):
                layer.cumulative_length.fill_(n)

    def capture(self, T):
        """two eager steps on a side stream, then the capture; the cache, the positions and the request's sampler state (its counter
        word, the `seen` set of its prompt) are re-set behind them"""
        from ._graphs import captured, warm_up
        s = self.sampler
        keep = (self.tok64.clone(), self.tok.clone(), s.counter.clone(), s.seen.clone() if s.seen is not None else None)
        warm_up(self.step, 2)
        self.graph = captured(self.step)
        # the warm-up steps wrote cache rows T-1 .. T+1 and moved the positions: rows past the position are overwritten before they are
        # read (causal), the rest is restored
        self.tok64.copy_(keep[0])
        self.tok.copy_(keep[1])
        s.reseed(keep[2])
        if s.seen is not None:  # (the warm-up steps left their draws in the set)
            s.seen.copy_(keep[3])
        self.pos.fill_(T - 1)
        if T == 1:  # (no prompt pass ran: the layers allocated their tensors inside the warm-up)
            self.cache.reset()
        self._set_cache_length(T - 1)

    def close(self):
        from ._graphs import release
        g, self.graph = self.graph, None
        release(g)
        self.cache = None


class AnyPrecisionForCausalLM(nn.Module):

    def __init__(self, model_path, config, precisions: Optional[List[int]] = None, torch_dtype=torch.float16, fuse_layers=False,
                 trust_remote_code=True, local_dir=None, device=None, random_init_seed: Optional[int] = None):
        super().__init__()
        from transformers import AutoModelForCausalLM
        if torch_dtype != torch.float16:
            raise RuntimeError('Only float16 is supported for now.')
        self.config = config
        self.model_path = model_path
        ap = config.anyprec if hasattr(config, "anyprec") else None
        if not ap:
            raise ValueError("config has no 'anyprec' section (not an Any-Precision checkpoint)")
        self.supported_bits = list(range(ap['seed_precision'], ap['parent_precision'] + 1))
        if precisions is None:
            self.precisions = self.supported_bits
        else:
            assert len(precisions) == len(set(precisions)), "Precisions must be unique"
            assert all(bit in self.supported_bits for bit in precisions), \
                f"Supported bits {precisions} must be a subset of model supported bits {self.supported_bits}"
            self.precisions = precisions
        self.precision = max(self.precisions)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)

        with torch.device("meta"):
            self.model = AutoModelForCausalLM.from_config(config=config, torch_dtype=torch_dtype, trust_remote_code=trust_remote_code)
        self.ap_linears = []
        self._load_quantized_modules()
        self._native_cache = {}
        self._released = None
        self.register_state_dict_pre_hook(lambda module, prefix, keep_vars: module._restore_module_tree())
        # (also when the HF model inside is asked directly: self.model.state_dict() / save_pretrained.  Through a weak reference -- the
        # wrapper owns captured graphs and must stay collectable by reference counting alone, see _graphs.py)
        self.model.register_state_dict_pre_hook(_WeakRestore(self))
        # new weights: the fused decode model (built from the old tensors) and every captured graph are stale
        self.register_load_state_dict_pre_hook(lambda module, *a, **k: module._drop_native())
        if random_init_seed is not None:
            self._random_weights(random_init_seed)
        else:
            if not os.path.exists(model_path):
                raise FileNotFoundError(f"{model_path}: not a local checkpoint directory (there is no hub download here; "
                                        "the reference calls snapshot_download)")
            self._load_weights(model_path)
        self.tie_weights()
        if self.device.type == "cuda":  # before transformers' generate captures anything under inference mode (generate.py)
            from .generate import prime_graph_rng_state
            prime_graph_rng_state(self.device)
        if fuse_layers:
            self.fuse_layers()
        self.prune_precisions()

    # -- construction ------------------------------------------------------------------------------------------------
    def get_model_layers(self):
        arch = (self.config.anyprec.get('arch_config') or {})
        module = _get_by_path(self.model, arch.get('model_name', 'model'))
        return getattr(module, arch.get('layers_name', 'layers'))

    @property
    def layer_type(self):
        for layer in self.get_model_layers():
            return layer.__class__.__name__
        return None

    def _load_quantized_modules(self):
        arch = (self.config.anyprec.get('arch_config') or {})
        names = arch.get('module_names')
        for layer in self.get_model_layers():
            targets = {}
            if names:
                for n in names:
                    targets[n] = _get_by_path(layer, n)
            else:
                targets = {n: m for n, m in layer.named_modules() if isinstance(m, nn.Linear)}
            for name, module in targets.items():
                lin = AnyPrecisionLinear(module.in_features, module.out_features, self.supported_bits, bias=module.bias is not None,
                                         precisions=self.precisions, device="meta", dtype=torch.float16)
                lin.output = torch.zeros((1, 1, module.out_features), dtype=torch.float16, device=self.device)
                self.ap_linears.append(lin)
                replace_module_by_name(layer, name, lin)

    def _materialise_meta_buffers(self):
        # non-persistent buffers (the rotary embedding's inv_freq) have no data in a checkpoint and are still on the meta
        # device: a fresh instance of the owning module, built from its config on the CPU, supplies them
        for mod in list(self.model.modules()):
            meta = [b for b, buf in mod._buffers.items() if buf is not None and buf.is_meta]
            if not meta:
                continue
            # (a scalar buffer whose value the module also keeps as a Python number: Gemma3's embedding scale, `scalar_embed_scale`)
            for b in [b for b in meta if hasattr(mod, "scalar_" + b)]:
                mod._buffers[b] = torch.tensor(getattr(mod, "scalar_" + b), dtype=mod._buffers[b].dtype)
                meta.remove(b)
            if not meta:
                continue
            if not hasattr(mod, "config"):
                raise RuntimeError(f"buffers {meta} of {type(mod).__name__} have no data in the checkpoint")
            with torch.device("cpu"):
                fresh = type(mod)(mod.config)
            for b in meta:
                mod._buffers[b] = fresh._buffers[b]

    def _random_weights(self, seed, lut_std=0.02):
        """synthetic weights of the checkpoint format, generated on the device (benchmarks / tests without a checkpoint on disk: the
        `--random_init` of inference/generate.py:222-245 for the HF-path harness)"""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        sd = {}
        for name, t in list(self.model.state_dict().items()):
            shape = tuple(t.shape)
            if name.endswith("qweight"):
                v = torch.randint(-2**31, 2**31 - 1, shape, dtype=torch.int32, device=self.device, generator=g)
            elif ".lut" in name:
                v = (torch.randn(shape, device=self.device, generator=g) * lut_std).sort(dim=1).values.half().contiguous()
            elif name.endswith("norm.weight") or "layernorm" in name:
                v = torch.ones(shape, dtype=torch.float16, device=self.device)
            else:
                v = (torch.randn(shape, device=self.device, generator=g) * 0.02).half()
            sd[name] = v
        self.model.load_state_dict(sd, strict=False, assign=True)
        self._materialise_meta_buffers()
        self.model.to(self.device)
        for lin in self.ap_linears:
            lin.output = lin.output.to(self.device)

    def _load_weights(self, path):
        sd = read_hf_state_dict(path)
        if "lm_head.weight" not in sd and getattr(self.config, "tie_word_embeddings", False):
            emb = [k for k in sd if k.endswith("embed_tokens.weight")]
            if emb:
                sd["lm_head.weight"] = sd[emb[0]]
        cast = {k: (v.to(torch.float16) if v.is_floating_point() else v) for k, v in sd.items()}
        missing, unexpected = self.model.load_state_dict(cast, strict=False, assign=True)
        missing = [k for k in missing if "rotary_emb.inv_freq" not in k]
        if missing:
            raise RuntimeError(f"checkpoint lacks {len(missing)} tensors, e.g. {missing[:4]}")
        self._materialise_meta_buffers()
        self.model.to(self.device)
        for lin in self.ap_linears:
            lin.output = lin.output.to(self.device)
        del sd, cast
        gc.collect()

    # -- the reference's surface ---------------------------------------------------------------------------------------
    def forward(self, *args, **kwargs):
        prev_precision = self.precision
        if 'precision' in kwargs:
            self.set_precision(kwargs.pop('precision'))
        results = self.model.forward(*args, **kwargs)
        self.set_precision(prev_precision)
        return results

    # keyword arguments of `generate` the fused routes understand (everything else -> transformers' own generate)
    _ROUTE_KW = {"input_ids", "inputs", "max_new_tokens", "min_new_tokens", "max_length", "do_sample", "temperature", "top_k", "top_p",
                 "pad_token_id", "eos_token_id", "attention_mask", "cache_implementation", "use_cache", "streamer", "num_beams",
                 "num_return_sequences", "repetition_penalty", "suppress_tokens", "return_dict_in_generate", "min_p"}

    def _route_request(self, args, kwargs, sampler_processors=False, full_sampler=False):
        """(params, None) when the request is one the fused decode routes serve -- ONE sequence, greedy or top-k (<= 64) sampling with
        or without a nucleus (top_p), no logits processors beyond min_new_tokens on EOS, a repetition penalty (finite, > 0) and
        suppress_tokens (a flat list of ids < vocab), both applied inside the fused sampler -- else (None, reason).
        sampler_processors: `generate` asks with True.  The two-argument form keeps the answer it always gave -- a repetition penalty
        other than 1 or a suppress list is declined -- for callers that drive a sampler without the token sets (gq_sample_topk_p).  Missing sampling arguments come from
        the model's generation_config exactly as in transformers (top_k defaults to 50 there).
        full_sampler: `generate` asks with True for route 1, whose sampler draws from the whole vocabulary (gq_sample_full): sampling without
        a top-k filter (top_k=0, or None from a transformers-4 style config) and min_p in (0, 1] (keyword or generation config) are then
        served.  top_k above 64 stays declined on this surface.  Without the flag the answers are the ones always given: no top_k, and
        any min_p, decline."""
        if len(args) > 1 or any(k not in self._ROUTE_KW for k in kwargs):
            return None, "arguments outside the fused routes: %s" % sorted(k for k in kwargs if k not in self._ROUTE_KW)
        ids = args[0] if args else kwargs.get("input_ids", kwargs.get("inputs"))
        if not torch.is_tensor(ids) or ids.dim() != 2 or ids.shape[0] != 1 or ids.shape[1] < 1 or ids.is_floating_point():
            return None, "input_ids must be one sequence of token ids, [1, T]"
        gc_ = getattr(self.model, "generation_config", None)

        # transformers 5 keeps unset fields of a GenerationConfig as None and fills in its global defaults at generate time (top_k = 50,
        # ...); in transformers 4 (the reference pins 4.52.3) the fields carry the defaults themselves and a None was put there by the
        # user (top_k=None: top-k filtering disabled)
        none_is_unset = gc_ is not None and hasattr(type(gc_), "_get_default_generation_params")

        def g(name, dflt=None):
            # a keyword that is not None wins, else the generation config's value, else the default
            v = kwargs.get(name)
            if v is not None:
                return v
            if gc_ is not None and hasattr(gc_, name):
                v = getattr(gc_, name)
                if v is not None or not none_is_unset:
                    return v
            return dflt
        if (g("num_beams", 1) or 1) != 1 or (g("num_return_sequences", 1) or 1) != 1 or g("return_dict_in_generate", False) or g("use_cache", True) is False:
            return None, "beam search / several return sequences / dict output / use_cache=False"
        rp = g("repetition_penalty", 1.0)
        try:  # (transformers demands a strictly positive float; the sampler a finite one)
            rp = 1.0 if rp is None else float(rp)
        except (TypeError, ValueError):
            return None, "repetition_penalty is not a number"
        if not (0.0 < rp < float("inf")):
            return None, "repetition_penalty must be finite and > 0"
        sup = g("suppress_tokens", None)
        if sup is None:
            sup = ()
        else:
            vocab = int(getattr(self.config, "vocab_size", 0) or 0)
            sup = sup.tolist() if torch.is_tensor(sup) and sup.dim() == 1 else sup
            if not isinstance(sup, (list, tuple)) or any(isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab for t in sup):
                return None, "suppress_tokens must be a flat list of token ids below the vocabulary size"
            sup = tuple(sorted(set(int(t) for t in sup)))
        if not sampler_processors and (rp != 1.0 or sup):
            return None, "repetition_penalty" if rp != 1.0 else "suppress_tokens"
        min_p = g("min_p", None)
        if min_p is not None and not isinstance(min_p, (int, float)):
            return None, "min_p is not a number"
        min_p = float(min_p or 0.0)
        if min_p != 0.0 and not full_sampler:
            return None, "min_p" if "min_p" in kwargs and kwargs["min_p"] is not None else "generation_config.min_p"
        if not 0.0 <= min_p <= 1.0:
            return None, "min_p outside [0, 1]"
        for name in ("no_repeat_ngram_size", "encoder_no_repeat_ngram_size", "bad_words_ids", "force_words_ids", "begin_suppress_tokens",
                     "forced_bos_token_id", "forced_eos_token_id", "sequence_bias", "typical_p", "epsilon_cutoff", "eta_cutoff", "penalty_alpha",
                     "min_length"):  # (min_p: above)
            v = getattr(gc_, name, None) if gc_ is not None else None
            if v not in (None, 0, 0.0, 1.0, [], False):
                return None, "generation_config.%s" % name
        T = int(ids.shape[1])
        max_new = g("max_new_tokens", None)  # (keyword first, then generation_config.max_new_tokens, then max_length - T: transformers' order)
        if max_new is None:
            ml = g("max_length", None)
            max_new = (int(ml) - T) if ml is not None else None
        if max_new is None or int(max_new) < 1:
            return None, "max_new_tokens"
        am = kwargs.get("attention_mask")
        if am is not None and not (tuple(am.shape) == tuple(ids.shape) and bool((am != 0).all())):
            return None, "attention_mask with masked positions"
        do_sample = bool(g("do_sample", False))
        temperature, top_k, top_p = 0.0, 1, 1.0
        if do_sample:
            t_ = g("temperature", 1.0)
            temperature = 1.0 if t_ is None else float(t_)
            top_p, top_k = g("top_p", 1.0), g("top_k", 50)
            top_p = 1.0 if top_p is None else float(top_p)
            if not 0.0 < top_p <= 1.0:
                return None, "top_p outside (0, 1]"
            # (round 6: top_p < 1 is served -- the fused sampler filters the nucleus of its top-k survivors the way transformers chains
            # TopKLogitsWarper and TopPLogitsWarper; without a top_k <= 64 the nucleus of the FULL distribution would be needed: declined)
            # (top_k None or 0 = no top-k filtering in transformers: the full distribution, which the 64-candidate sampler does not draw from)
            # (full_sampler: no top-k filter is served by the whole-vocabulary sampler; 65.. stays declined on this surface)
            if full_sampler and not top_k and temperature > 0.0:
                top_k = 0
            elif not top_k or int(top_k) < 1 or int(top_k) > 64 or temperature <= 0.0:
                return None, "top_k outside 1..64 (the fused sampler's candidates)"
        else:
            min_p = 0.0  # (greedy: transformers applies no warper)
        eos = g("eos_token_id", None)
        eos = [] if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
        if len(eos) > 4:
            return None, "more than 4 EOS ids"
        return dict(ids=ids, T=T, max_new=int(max_new), min_new=min(int(g("min_new_tokens", 0) or 0), int(max_new)), temperature=temperature,
                    top_k=int(top_k), top_p=float(top_p), eos=eos, streamer=kwargs.get("streamer"), do_sample=do_sample,
                    repetition_penalty=rp, suppress_tokens=sup, min_p=min_p), None

    def generate(self, *args, **kwargs):
        """`generate` of the reference's HF surface (inference_example.py:34-77).  Three routes behind the one call:
          1. the fused decode model of the same checkpoint (`native_decoder`: prompt through the HIP prompt pass, every new token one
             replay of the captured 5-launches-per-layer graph, sampling / EOS suppression / embedding of the next token on the device)
             -- taken AUTOMATICALLY for a request it serves (`_route_request`: one sequence, greedy or sampling with top_k in 1..64 or
             with NO top-k filter (top_k=0, or None in a transformers-4 style config), with or without a nucleus top_p and min_p,
             min_new_tokens, repetition_penalty, suppress_tokens -- the reference's own call and the published Qwen2.5-Instruct
             generation config).  Without a top-k filter, or with min_p, the step ends in the whole-vocabulary sampler (gq_sample_full);
             top_k above 64 is NOT served on this surface yet (tests/test_hf_routes_gpu.py pins that it raises with native=True; lifting
             it is a follow-up) -- `DecodeGraph(native_sampling=True, top_k=200)` serves it; `native=False` opts out, `native=True` insists (ValueError when the request is not
             served).  The automatic route keeps the module tree whole, so the fused q/k/v/gate/up tensors are a SECOND copy of those
             weights on the device (1.1 GB for an 8B 2-bit model, about 14 GB for a 70B one; see `native_decoder`); `native=True` releases the module tree's copy;
          2. `capture=True`: the HF module tree with its decode step captured as ONE hipGraph over a transformers StaticCache, the
             fused sampler at its end -- opt-in: measured SLOWER than route 3 on the 8B model (172 vs 249 tokens/s: the module tree's
             ~1,500 small launches per token cost more as graph nodes than as stream launches; the fused model is the fast form);
          3. transformers' own generate on the module tree (anything else: beams, top_k > 64, other logits processors, batches,
             dict output; or `native=False`).
        Route 1 serves every precision of the checkpoint, 2 to 8 bits: the decode step's GEMVs run the exact fp16-order kernels
        below 5 bits and ap_wide.hip's LDS-table kernel from 5 to 8 (a parent of 8 bits serves precision=5..8 without the module tree).
        repetition_penalty (finite, > 0; keyword or generation config) and suppress_tokens (a flat list of ids) are applied INSIDE the
        fused sampler of routes 1 and 2, as transformers applies RepetitionPenaltyLogitsProcessor and SuppressTokensLogitsProcessor to the
        fp32 scores: a token of the sequence so far (prompt included) has its logit divided by the penalty when positive and multiplied
        when negative, once per distinct token; a suppressed token is never drawn (and, stricter than -inf, takes no top_k place).
        Prompt length on route 1: prompt + max_new_tokens up to the decoder's `block_size` (the checkpoint's max_position_embeddings) --
        a prompt of more than GQ_PREFILL_CHUNK (4096) tokens goes through the chunked HIP prompt pass (`Transformer.prefill_native`),
        its intermediates sized by the chunk and its attention by gq_attn_prefill; the caches keep no quadratic mask table.
        Returns the [1, prompt + new] token tensor like HF does; stops at EOS (checked every 32 tokens, the tail is cut); honours
        min_new_tokens, streamer, precision=.
        output_logprobs=True (route 1 only; `native=False`, `capture=True` or a request route 1 does not serve raise ValueError, it never
        falls back): returns a `GenerateLogprobsOutput` instead -- `sequences` (the tensor the call returns without the keyword),
        `logprobs` fp32 [1, new]: the log-probability of every generated token under the model's unprocessed distribution, as `score`
        defines it for given text but from the logits of the decode step the token was drawn at; and `sampled_logprobs` fp32 [1, new]:
        under the distribution the draw was made from (after repetition penalty, suppress list, temperature, top-k and top-p; 0 for a
        greedy request) -- transformers' compute_transition_scores(normalize_logits=True).  `logprobs[0, j]` belongs to
        `sequences[0, T + j]`; both are cut at EOS where the sequence is.  The fused sampler writes them in the launch that draws the
        token (gq_sample_topk_lp): no [steps, vocab] scores are kept.
        top_logprobs=n, 1..20 (with output_logprobs=True only; without it, with n outside the range, `native=False`, `capture=True` or a
        request route 1 does not serve: ValueError, never a fall-back, and the keyword never reaches transformers): the output gains
        `top_logprobs_ids` int64 [1, new, n] -- the n most probable tokens of the model's UNPROCESSED distribution at each step, most
        probable first, equal logits by ascending id, -1 where the vocabulary has fewer -- and `top_logprobs` fp32 [1, new, n], their
        log-probabilities against the log-sum-exp `logprobs` is taken against: where the drawn token is listed its entry equals
        `logprobs[0, j]` bit for bit.  Penalty, suppress list, min_new_tokens' EOS ban, temperature and the filters do not enter the list.
        Both are cut at EOS where `sequences` is.  Two launches per token behind the sampler's (csrc/topn.hip).
        lm_head_dtype="int8" (route 1 only; `native=False`, `capture=True`, the CPU, or a request or checkpoint route 1 declines raise
        ValueError("lm_head_dtype='int8': ..."), never a fall-back, and the keyword never reaches transformers): the decode step's head
        reads a weight-only int8 copy of the lm_head with one fp32 scale per row (gq_dense_gemv_i8; `Transformer.set_lm_head_dtype`:
        N*K + 4N bytes next to the fp16 head, which the prompt pass and `score` keep reading).  None / "fp16": a call without the keyword;
        a request without it switches the decoder back and frees the copy.
        frequency_penalty / presence_penalty (finite numbers) and logit_bias ({token id: finite bias}; the ids as ints or, as serving APIs
        send them, as strings) -- route 1 only; `native=False`, `capture=True` or a request route 1 declines raise
        ValueError("frequency_penalty: ...") (the name of the first of the three that is active), never a fall-back, and the keywords never
        reach transformers: a serving API's additive adjustments inside the fused sampler's launches (gq_sample_topk_adj /
        gq_sample_full_adj).  For a token with a listed bias b, or one THIS request has generated c > 0 times, the logit v becomes
        fp16((v + b) - (c > 0 ? frequency_penalty * c + presence_penalty : 0)), every operation rounded in fp32 and the result to fp16;
        every other token keeps its logit.  The prompt does not count (OpenAI's / vLLM's meaning; repetition_penalty, transformers'
        processor, does include it).  They are logits processors, not warpers: a greedy request applies them too.  The additive terms
        come first and the repetition penalty behind them (vLLM penalises repetition first); transformers' sequence_bias adds to fp32
        scores without the rounding to fp16.  `logprobs` and `top_logprobs` stay the unprocessed distribution's, `sampled_logprobs`
        sees the adjustment.  0, 0 and None / {}: a call without the keywords.
        token_fsm=a `token_fsm.TokenFSM` (route 1 only; `native=False`, `capture=True`, a request route 1 declines, or min_new_tokens > 0 --
        an EOS-only state under the ban would be empty -- raise ValueError("token_fsm: ..."), never a fall-back, and the keyword never
        reaches transformers): constrained decoding inside the fused sampler's launches (gq_sample_topk_fsm / gq_sample_full_fsm).  Every
        generated token is one the machine's current state allows -- the state's forbidden set stands in for the suppress list, so a
        forbidden token takes no top_k place and `sampled_logprobs` is under the masked distribution -- and the drawn token moves the
        state on the device: no host callback per token, and the multi-step replays keep working.  Every request starts in the machine's
        start state.  `logprobs` and `top_logprobs` stay the unprocessed distribution's; the penalties, the suppress list and the bias
        compose unchanged.  The decoder's sampler is keyed on the machine's content.  None: a call without the keyword."""
        prev_precision = self.precision
        if 'precision' in kwargs:
            self.set_precision(kwargs.pop('precision'))
        native = kwargs.pop('native', None)
        capture = kwargs.pop('capture', None)
        # kv_cache_dtype="fp8": the KV cache of the fused decode model as e4m3 codes (Transformer.setup_caches).  Served by route 1 only;
        # a request it cannot serve raises -- it never falls back to an fp16 cache silently.  (popped: it never reaches transformers)
        from .model import kv_cache_dtype_name
        kv = kv_cache_dtype_name(kwargs.pop('kv_cache_dtype', None))
        # lm_head_dtype="int8": the fused decode step's head over a weight-only int8 copy (Transformer.set_lm_head_dtype).  Route 1 only,
        # never a fall-back; None / "fp16" is a call without the keyword.  (popped as well; validated inside the try)
        hd = kwargs.pop('lm_head_dtype', None)
        # output_logprobs=True: per-token log-probabilities from the fused sampler.  Route 1 only, never a fall-back.  (popped as well)
        lp = bool(kwargs.pop('output_logprobs', False))
        top_n = kwargs.pop('top_logprobs', None)  # (popped as well; validated inside the try: the precision is restored on a refusal)
        # frequency_penalty / presence_penalty / logit_bias: additive adjustments inside the fused sampler.  Route 1 only, never a fall-back.
        adj = {k: kwargs.pop(k, None) for k in ("frequency_penalty", "presence_penalty", "logit_bias")}  # (popped as well; validated inside the try)
        fsm = kwargs.pop("token_fsm", None)  # (popped as well; validated inside the try)
        try:
            from .fused_sampler import check_additive_penalty, check_logit_bias
            adj = dict(frequency_penalty=check_additive_penalty("frequency_penalty", adj["frequency_penalty"]),
                       presence_penalty=check_additive_penalty("presence_penalty", adj["presence_penalty"]),
                       logit_bias=check_logit_bias(adj["logit_bias"], int(getattr(self.config, "vocab_size", 0) or 0)))
            adj = {k: v for k, v in adj.items() if v}  # (the active ones; the first names the refusals below)
            if fsm is not None:  # (the machine rides with the adjustments: the same route, the same refusals under its own name)
                from .token_fsm import TokenFSM
                if not isinstance(fsm, TokenFSM):
                    raise ValueError(f"token_fsm: must be a guidedquant_amd.token_fsm.TokenFSM, not {type(fsm).__name__}")
                try:
                    fsm.check(int(getattr(self.config, "vocab_size", 0) or 0))
                except ValueError as e:
                    raise ValueError("token_fsm: " + str(e).removeprefix("token_fsm: ")) from None
                adj = {"token_fsm": fsm, **adj}
            adj_name = next(iter(adj), None)
            if adj_name and (native is False or capture is True):
                raise ValueError(f"{adj_name}: served by the fused decode model only (not with native=False or capture=True)")
            from .fused_sampler import check_top_logprobs
            if top_n is not None and not check_top_logprobs(top_n, lp):  # (the keyword, once given, asks for a list: None alone is "off" here)
                raise ValueError(f"top_logprobs must be an integer in 1..20, not {top_n!r}")
            top_n = int(top_n or 0)  # (top_n > 0 implies lp: every refusal of output_logprobs below is one of top_logprobs)
            from .head_q8 import lm_head_dtype_name
            hd = lm_head_dtype_name(hd)
            if hd == "int8" and (native is False or capture is True):
                raise ValueError("lm_head_dtype='int8': served by the fused decode model only (not with native=False or capture=True)")
            if lp and (native is False or capture is True):
                raise ValueError("output_logprobs=True: served by the fused decode model only (not with native=False or capture=True)")
            if kv == "fp8" and (native is False or capture is True):
                raise ValueError("kv_cache_dtype='fp8': served by the fused decode model only (not with native=False or capture=True)")
            # (full_sampler: route 1's sampler draws from the whole vocabulary; route 2 keeps the 64-candidate kernels and their answers)
            req, why = self._route_request(args, kwargs, sampler_processors=True, full_sampler=capture is not True) \
                if (native is not False or capture is True) else (None, "opted out")
            if req is not None and self.device.type != "cuda":
                req, why = None, "the fused routes need the GPU"
            if kv == "fp8" and req is None:
                raise ValueError("kv_cache_dtype='fp8': " + why)
            if hd == "int8" and req is None:
                raise ValueError("lm_head_dtype='int8': " + why)
            if lp and req is None:
                raise ValueError("output_logprobs=True: " + why)
            if adj_name and req is None:
                raise ValueError(f"{adj_name}: " + why)
            if fsm is not None and req["min_new"] > 0:
                raise ValueError("token_fsm: not served together with min_new_tokens > 0 (a state that allows only EOS would be empty under the ban)")
            if native is True and req is None:
                raise ValueError("native=True: " + why)
            if req is not None and native is not False:
                # (the q/k/v/gate/up planes of the module tree are released only on the explicit native=True: the automatic route keeps
                # the module tree whole, so that model.state_dict() / save_pretrained / direct buffer access after a plain generate()
                # see every tensor)
                dec = self._native_decoder_or_none(self.precision, release_planes=native is True)
                if dec is not None and req["T"] + req["max_new"] > dec.config.block_size:
                    if hd == "int8":
                        raise ValueError(f"lm_head_dtype='int8': prompt + max_new_tokens = {req['T'] + req['max_new']} exceeds the fused "
                                         f"model's context ({dec.config.block_size})")
                    if lp:
                        raise ValueError(f"output_logprobs=True: prompt + max_new_tokens = {req['T'] + req['max_new']} exceeds the fused "
                                         f"model's context ({dec.config.block_size})")
                    if adj_name:
                        raise ValueError(f"{adj_name}: prompt + max_new_tokens = {req['T'] + req['max_new']} exceeds the fused model's "
                                         f"context ({dec.config.block_size})")
                    if native is True:
                        raise ValueError(f"native=True: prompt + max_new_tokens = {req['T'] + req['max_new']} exceeds the fused model's "
                                         f"context ({dec.config.block_size})")
                    dec = None  # (automatic route: transformers' generate decides what a request beyond the context means)
                from ._lib import SAMPLER_MAX_VOCAB
                if dec is not None and dec.config.vocab_size > SAMPLER_MAX_VOCAB:
                    # (the captured step ends in the fused sampler: 128 blocks x 2048 logits at the most.  Qwen3's published vocabulary,
                    # 151936, is within it; a checkpoint beyond 262144 keeps `native_decoder()` / `decode_native` / `prefill_native`,
                    # not this route)
                    if hd == "int8":
                        raise ValueError(f"lm_head_dtype='int8': vocabulary {dec.config.vocab_size} exceeds the fused sampler's {SAMPLER_MAX_VOCAB}")
                    if lp:
                        raise ValueError(f"output_logprobs=True: vocabulary {dec.config.vocab_size} exceeds the fused sampler's {SAMPLER_MAX_VOCAB}")
                    if adj_name:
                        raise ValueError(f"{adj_name}: vocabulary {dec.config.vocab_size} exceeds the fused sampler's {SAMPLER_MAX_VOCAB}")
                    if native is True:
                        raise ValueError(f"native=True: vocabulary {dec.config.vocab_size} exceeds the fused sampler's {SAMPLER_MAX_VOCAB}")
                    dec = None
                if dec is not None and kv == "fp8" and dec.kv8_unserved():
                    raise ValueError("kv_cache_dtype='fp8': " + dec.kv8_unserved())
                if dec is not None:
                    return self._generate_native(dec, req, kv_cache_dtype=kv, logprobs=lp, top_logprobs=top_n, lm_head_dtype=hd, adjust=adj)
                if hd == "int8":
                    why_not = getattr(self, "_no_native_reason", None)
                    raise ValueError("lm_head_dtype='int8': this checkpoint has no fused decode form at %d bits%s" % (self.precision, ": " + why_not if why_not else ""))
                if lp:
                    why_not = getattr(self, "_no_native_reason", None)
                    raise ValueError("output_logprobs=True: this checkpoint has no fused decode form at %d bits%s" % (self.precision, ": " + why_not if why_not else ""))
                if adj_name:
                    why_not = getattr(self, "_no_native_reason", None)
                    raise ValueError("%s: this checkpoint has no fused decode form at %d bits%s" % (adj_name, self.precision, ": " + why_not if why_not else ""))
                if kv == "fp8":
                    why_not = getattr(self, "_no_native_reason", None)
                    raise ValueError("kv_cache_dtype='fp8': no fused decode model serves this request%s" % (": " + why_not if why_not else " (context or vocabulary beyond it)"))
                if native is True:
                    why_not = getattr(self, "_no_native_reason", None)
                    raise ValueError("native=True: this checkpoint has no fused decode form at %d bits%s" % (self.precision, ": " + why_not if why_not else ""))
            if capture is True:
                if req is None:
                    raise ValueError("capture=True: " + why)
                return self._generate_captured(req)
            with torch.inference_mode():
                return self.model.generate(*args, **kwargs)
        finally:
            self.set_precision(prev_precision)

    # -- scoring: log-likelihood and perplexity of given token ids ------------------------------------------------------
    @staticmethod
    def _score_rows(logits, targets, rows=512):
        """(logprob fp32 [n], top1 [n]) of logits [n, V] and targets [n]: float -> log_softmax -> gather / argmax in blocks of `rows`
        rows (the torch scoring head of Transformer._score_head; HF's loss upcasts the same way)"""
        lps, tops = [], []
        for a in range(0, logits.shape[0], rows):
            ls = torch.nn.functional.log_softmax(logits[a:a + rows].float(), dim=-1)
            lps.append(ls.gather(1, targets[a:a + rows, None])[:, 0])
            tops.append(ls.argmax(dim=-1))
        return torch.cat(lps), torch.cat(tops)

    def score(self, input_ids, precision=None, kv_cache_dtype=None, native=None):
        """Log-probabilities of one token sequence ([1, T] or [T], T >= 2): dict(logprobs fp32 [T - 1], greedy bool [T - 1], nll float)
        with logprobs[i] = log p(ids[i + 1] | ids[:i + 1]), greedy[i] = (the most probable next token is ids[i + 1]) and nll the mean of
        -logprobs -- the `outputs.loss` of the module tree for `labels=input_ids` (any_precision/evaluate/eval.py:222-223).
        Routing follows `generate`: the fused decode model's HIP prompt pass with the scoring head (`Transformer.score_native`: no
        [T, V] logits in memory) when the checkpoint has one at this precision and T fits its context, else the module tree's forward
        and the same formula in torch.  native=False opts out, native=True raises instead of falling back, and
        kv_cache_dtype="fp8" (the fused model's e4m3 cache) never falls back silently.  Ids outside [0, vocab) raise ValueError before
        anything is launched."""
        from .model import kv_cache_dtype_name
        kv = kv_cache_dtype_name(kv_cache_dtype)
        ids = torch.as_tensor(input_ids)
        if ids.is_floating_point() or ids.dim() not in (1, 2) or (ids.dim() == 2 and ids.shape[0] != 1):
            raise ValueError("score: input_ids must be one sequence of token ids, [1, T] or [T]")
        ids = ids.reshape(-1)
        T = int(ids.numel())
        if T < 2:
            raise ValueError("score: at least two tokens (the first one is only ever context)")
        host = ids.cpu()
        vocab = int(self.config.vocab_size)
        if int(host.min()) < 0 or int(host.max()) >= vocab:
            raise ValueError(f"score: token ids must lie in [0, {vocab})")
        if kv == "fp8" and native is False:
            raise ValueError("kv_cache_dtype='fp8': served by the fused decode model only (not with native=False)")
        prev_precision = self.precision
        if precision is not None:
            self.set_precision(precision)
        try:
            dec, why = None, "opted out"
            if native is not False:
                if self.device.type != "cuda":
                    why = "the fused routes need the GPU"
                else:
                    dec = self._native_decoder_or_none(self.precision, release_planes=native is True)
                    why = getattr(self, "_no_native_reason", None) or "this checkpoint has no fused decode form at %d bits" % self.precision
                    if dec is not None and T > dec.config.block_size:
                        dec, why = None, f"{T} tokens exceed the fused model's context ({dec.config.block_size})"
                    if dec is not None and kv == "fp8" and dec.kv8_unserved():
                        dec, why = None, dec.kv8_unserved()
                    if dec is not None and not dec.prefill_ready(ids.to(self.device).to(torch.int32)):
                        dec, why = None, "the fused model's prompt pass does not serve this model"
            if dec is None and kv == "fp8":
                raise ValueError("kv_cache_dtype='fp8': " + why)
            if dec is None and native is True:
                raise ValueError("native=True: " + why)
            if dec is not None:
                # the caches sized as `_generate_native` sizes them, and like there allocated OUTSIDE inference mode (tensors made inside
                # it refuse in-place updates elsewhere: set_kv_scales, the module forward's cache write); graphs captured over caches
                # about to be replaced go first
                cap = min(T if T > 16384 else max(256, 1 << (T - 1).bit_length()), dec.config.block_size)
                if not (dec.max_seq_length >= cap and dec.max_batch_size >= 1 and dec.kv_cache_dtype == kv):
                    self._evict("graph")
                dec.setup_caches(1, cap, kv_cache_dtype=kv)
            with torch.inference_mode():
                if dec is not None:
                    lp, greedy = dec.score_native(ids.to(self.device).to(torch.int32))
                else:
                    dev_ids = ids.to(self.device).long()
                    logits = self.model(input_ids=dev_ids.view(1, -1)).logits[0, :-1]
                    lp, top1 = self._score_rows(logits, dev_ids[1:])
                    greedy = top1 == dev_ids[1:]
            return dict(logprobs=lp, greedy=greedy, nll=float(-lp.double().mean()))
        finally:
            self.set_precision(prev_precision)

    def perplexity(self, token_ids, chunk_size=2048, **score_kwargs):
        """Perplexity of a 1-D token stream by the reference's definition (any_precision/evaluate/eval.py:205-226): the stream is cut
        into len // chunk_size non-overlapping chunks (a shorter tail is dropped), each chunk's mean negative log-likelihood is taken
        on its own (`score`; its first token is context only), and the result is exp of the mean of those means.
        Returns dict(ppl, nll_per_chunk).  `score_kwargs` (precision, kv_cache_dtype, native) go to `score`."""
        ids = torch.as_tensor(token_ids)
        if ids.dim() != 1:
            raise ValueError("perplexity: token_ids must be a 1-D stream of token ids")
        chunk_size = int(chunk_size)
        n = int(ids.numel()) // chunk_size if chunk_size >= 2 else 0
        if n < 1:
            raise ValueError(f"perplexity: chunk_size >= 2 and at least one whole chunk of {chunk_size} tokens")
        nlls = [self.score(ids[i * chunk_size:(i + 1) * chunk_size], **score_kwargs)["nll"] for i in range(n)]
        import math
        return dict(ppl=math.exp(sum(nlls) / n), nll_per_chunk=nlls)

    def loglikelihood(self, context_ids, continuation_ids, **score_kwargs):
        """lm-eval's pair for a (context, continuation): (the sum of the continuation tokens' log-probabilities given everything in
        front of them, whether every one of them is the model's most probable token), from ONE pass over context + continuation."""
        ctx, cont = torch.as_tensor(context_ids).reshape(-1), torch.as_tensor(continuation_ids).reshape(-1)
        if ctx.numel() < 1 or cont.numel() < 1:
            raise ValueError("loglikelihood: a context and a continuation of at least one token each")
        r = self.score(torch.cat([ctx.cpu(), cont.cpu()]), **score_kwargs)
        k = int(cont.numel())
        return float(r["logprobs"][-k:].double().sum()), bool(r["greedy"][-k:].all())

    # -- scoring many sequences: packs of short sequences through one prompt pass each ----------------------------------------
    def _checked_ids(self, input_ids, what):
        """`score`'s validation of one sequence: its ids as a 1-D host tensor"""
        ids = torch.as_tensor(input_ids)
        if ids.is_floating_point() or ids.dim() not in (1, 2) or (ids.dim() == 2 and ids.shape[0] != 1):
            raise ValueError(f"{what}: every sequence must be token ids, [1, T] or [T]")
        host = ids.reshape(-1).cpu()
        if int(host.numel()) < 2:
            raise ValueError(f"{what}: at least two tokens per sequence (the first one is only ever context)")
        vocab = int(self.config.vocab_size)
        if int(host.min()) < 0 or int(host.max()) >= vocab:
            raise ValueError(f"{what}: token ids must lie in [0, {vocab})")
        return host

    def _score_packs(self, seqs, tails, pack_tokens, precision, native, what):
        """[(logprobs fp32 [t_i], greedy bool [t_i])] in input order: the last `tails[i]` log-probabilities of sequence i (None: all of its
        T_i - 1).  On the fused route the sequences go through `Transformer.score_packed_native` in packs (native_prompt.pack_plan: first
        fit in input order), and only the rows asked for reach the scoring head; a sequence longer than a pack, and every sequence off the
        fused route, goes through `score`."""
        if pack_tokens is not None and int(pack_tokens) < 2:
            raise ValueError(f"{what}: pack_tokens must be at least 2")
        from . import native_prompt

        def tail(lp, greedy, t):
            return (lp, greedy) if t is None else (lp[-t:], greedy[-t:])
        prev_precision = self.precision
        if precision is not None:
            self.set_precision(precision)
        try:
            dec, why = None, "opted out"
            if native is not False:
                if self.device.type != "cuda":
                    why = "the fused routes need the GPU"
                else:
                    dec = self._native_decoder_or_none(self.precision, release_planes=native is True)
                    why = getattr(self, "_no_native_reason", None) or "this checkpoint has no fused decode form at %d bits" % self.precision
                    longest = max((int(s.numel()) for s in seqs), default=0)
                    if dec is not None and longest > dec.config.block_size:
                        dec, why = None, f"{longest} tokens exceed the fused model's context ({dec.config.block_size})"
                    if dec is not None and seqs and not dec.prefill_ready(seqs[0].to(self.device).to(torch.int32)):
                        dec, why = None, "the fused model's prompt pass does not serve this model"
            if dec is None and native is True:
                raise ValueError("native=True: " + why)
            if dec is None:
                out = []
                for s, t in zip(seqs, tails):
                    r = self.score(s, native=native)
                    out.append(tail(r["logprobs"], r["greedy"], t))
                return out
            capacity = native_prompt.pack_capacity(dec) if pack_tokens is None else min(int(pack_tokens), int(dec.config.block_size))
            lens = [int(s.numel()) for s in seqs]
            packs = native_prompt.pack_plan(lens, capacity)
            out = [None] * len(seqs)
            rows_max = max((sum(lens[i] for i in p) for p in packs if sum(lens[i] for i in p) <= capacity), default=0)
            if rows_max:
                # (the caches as `score` sizes them, allocated outside inference mode; graphs captured over caches about to be replaced go first)
                cap = min(max(256, 1 << (rows_max - 1).bit_length()), dec.config.block_size)
                if not (dec.max_seq_length >= cap and dec.max_batch_size >= 1 and dec.kv_cache_dtype == "fp16"):
                    self._evict("graph")
                dec.setup_caches(1, cap, kv_cache_dtype="fp16")
            for p in packs:
                if sum(lens[i] for i in p) > capacity:  # (one sequence longer than a pack: the one-sequence pass, chunked as it is there)
                    r = self.score(seqs[p[0]], native=native)
                    out[p[0]] = tail(r["logprobs"], r["greedy"], tails[p[0]])
                    continue
                dev_seqs = [seqs[i].to(self.device).to(torch.int32) for i in p]
                rows, counts = None, [lens[i] - 1 if tails[i] is None else tails[i] for i in p]
                if any(tails[i] is not None for i in p):
                    mask, b = torch.zeros(sum(lens[i] for i in p), dtype=torch.bool), 0
                    for i, c in zip(p, counts):
                        mask[b + lens[i] - 1 - c:b + lens[i] - 1] = True
                        b += lens[i]
                    rows = mask.to(self.device)
                with torch.inference_mode():
                    lp, hit = dec.score_packed_native(dev_seqs, rows)
                b = 0
                for i, c in zip(p, counts):
                    out[i] = (lp[b:b + c], hit[b:b + c])
                    b += lens[i] if rows is None else c  # (rows None: the head ran on every row, and a sequence's last row is no prediction)
            return out
        finally:
            self.set_precision(prev_precision)

    def score_many(self, list_of_ids, pack_tokens=None, precision=None, native=None):
        """`score` for many sequences: a list of its dicts (logprobs fp32 [T_i - 1], greedy bool [T_i - 1], nll float) in input order.
        On the fused route the sequences are packed -- first fit in input order into packs of at most `pack_tokens` rows (default: the
        smaller of GQ_PREFILL_CHUNK and the model's context) -- and every pack is ONE prompt pass (`Transformer.score_packed_native`:
        varlen attention, the weights read once per pack instead of once per sequence); a sequence longer than a pack goes through
        `score`.  A packed result is a rounding of the same model as `score`'s, not bit-equal to it: the GEMMs see other row counts.
        Validation, `precision` and `native` as in `score`: off the fused route (native=False, no fused form, the CPU) this is a loop
        over `score`, and native=True raises instead of falling back.  fp16 KV cache."""
        seqs = [self._checked_ids(ids, "score_many") for ids in list_of_ids]
        res = self._score_packs(seqs, [None] * len(seqs), pack_tokens, precision, native, "score_many")
        return [dict(logprobs=lp, greedy=g, nll=float(-lp.double().mean())) for lp, g in res]

    def loglikelihood_many(self, pairs, pack_tokens=None, precision=None, native=None):
        """`loglikelihood` for many (context, continuation) pairs -- the requests lm-eval issues by the thousand: a list of (sum of the
        continuation's log-probabilities, all of them greedy) in input order, packed like `score_many`.  Only the rows that predict a
        continuation token reach the final norm and the lm_head."""
        seqs, tails = [], []
        for ctx, cont in pairs:
            ctx, cont = torch.as_tensor(ctx).reshape(-1), torch.as_tensor(cont).reshape(-1)
            if ctx.numel() < 1 or cont.numel() < 1:
                raise ValueError("loglikelihood_many: a context and a continuation of at least one token each")
            seqs.append(self._checked_ids(torch.cat([ctx.cpu(), cont.cpu()]), "loglikelihood_many"))
            tails.append(int(cont.numel()))
        res = self._score_packs(seqs, tails, pack_tokens, precision, native, "loglikelihood_many")
        return [(float(lp.double().sum()), bool(g.all())) for lp, g in res]

    # -- route 1: the fused decode model ---------------------------------------------------------------------------------
    _SAMPLER_SEED = 0x2545F491  # (a constant: what varies between sampled calls is the counter word, drawn from torch's generator)

    def _fresh_rng_word(self):
        """the start of the fused sampler's counter stream for ONE sampled call, drawn from torch's generator of this device: as with
        transformers' generate, `torch.manual_seed(s)` before a call makes it reproducible and two unseeded calls differ -- whatever
        graph is cached (the captured launches read the counter from device memory, nothing of the seed is baked in)"""
        return torch.randint(-2**31, 2**31 - 1, (1, ), dtype=torch.int32, device=self.device)

    def _native_decoder_or_none(self, bitwidth, release_planes=False):
        try:
            dec = self.native_decoder(bitwidth, release_planes=release_planes)
        except (ValueError, NotImplementedError) as e:  # "this checkpoint / precision has no fused form"; anything else is a real error
            self._no_native_reason = str(e)
            return None
        self._no_native_reason = None
        dec.setup_caches(1, 8, kv_cache_dtype=dec.kv_cache_dtype) if not dec.cache_initialized else None
        return dec if dec.native_ready() else None

    def _evict(self, kind):
        """drop the cached entries of one kind ("graph": DecodeGraphs of route 1, "cap": captured steps of route 2), destroying their
        hipGraphs synchronously -- never left to a finaliser that may run inside a later capture (_graphs.py)"""
        keep = {}
        for k, v in self._native_cache.items():
            if k[0] == kind:
                v.close()
            else:
                keep[k] = v
        self._native_cache = keep

    def _emit(self, req, seq_host, lo, hi):
        """tokens [lo, hi) of the host copy of the sequence: to the streamer (up to and including the first EOS that counts -- index
        >= T + min_new_tokens); returns the index behind that EOS, or None"""
        cut = None
        for i in range(max(lo, req["T"] + req["min_new"]), hi if req["eos"] else 0):
            if int(seq_host[i]) in req["eos"]:
                cut = i + 1
                break
        if req["streamer"] is not None and hi > lo:
            req["streamer"].put(seq_host[lo:(cut or hi)])
        return cut

    def _run_request(self, req, ids, sampler, run, chunk=32, logprobs=False, top_logprobs=0):
        """One request on a fused route, from the point where the caches hold the prompt but for its last token and that token and its
        position are set: the sampler's per-request state (the sequence prefix, the `ban` words of min_new_tokens, a fresh counter word
        for a sampled call, the `seen` set of the prompt), then `run(n)` -- n token steps of the route -- in chunks of `chunk` tokens with
        the EOS check and the streamer in between; returns what `generate` returns."""
        T, max_new = req["T"], req["max_new"]
        ids32 = ids.view(-1).to(torch.int32)
        sampler.seq[:T].copy_(ids32)
        # EOS cannot be drawn before min_new_tokens are out: the token of the step at position p is new token number p + 2 - T
        sampler.set_ban(req["eos"], T - 1 + req["min_new"])
        if req.get("do_sample"):
            sampler.reseed(self._fresh_rng_word())
        sampler.set_history(ids32)  # (the penalty's token set: all T prompt tokens, rebuilt per request)
        sampler.reset_generated()  # (the counts of a frequency / presence penalty: this request has generated nothing yet)
        sampler.reset_fsm()  # (a token_fsm: the machine is in its start state)
        if req["streamer"] is not None:
            req["streamer"].put(ids.cpu())
        done, cut = 0, None
        host_checks = bool(req["eos"]) and req["min_new"] < max_new or req["streamer"] is not None
        while done < max_new and cut is None:
            n = min(chunk, max_new - done) if host_checks else max_new - done
            run(n)
            if host_checks:
                seq_host = sampler.seq[:T + done + n].cpu().long()
                cut = self._emit(req, seq_host, T + done, T + done + n)
            done += n
        end = cut if cut is not None else T + done
        out = sampler.seq[:end].to(ids.dtype).view(1, -1).clone()
        if logprobs:  # (slot i of the two arrays describes seq[i]: the sampler's index)
            out = GenerateLogprobsOutput(sequences=out, logprobs=sampler.lp_raw[T:end].view(1, -1).clone(),
                                         sampled_logprobs=sampler.lp_drawn[T:end].view(1, -1).clone(),
                                         **(dict(top_logprobs_ids=sampler.top_ids[T:end].long().unsqueeze(0), top_logprobs=sampler.top_lps[T:end].unsqueeze(0).clone())
                                            if top_logprobs else {}))
        if req["streamer"] is not None:
            req["streamer"].end()
        return out

    def _generate_native(self, dec, req, chunk=32, kv_cache_dtype="fp16", logprobs=False, top_logprobs=0, lm_head_dtype="fp16", adjust=None):
        from . import generate as gen
        ids, T, max_new = req["ids"].to(self.device), req["T"], req["max_new"]
        total = T + max_new
        if total > dec.config.block_size:
            raise ValueError(f"prompt + max_new_tokens = {total} exceeds the model's context ({dec.config.block_size})")
        # caches (and with them the captured graphs, keyed by the cache length) grow in powers of two from 256 positions: a serving loop
        # with varying lengths re-captures at most log2 times, not per request (the attention launch reads rows up to the position
        # only; a longer cache costs memory, not time).  Beyond 16384 positions the request's own length.
        cap = total if total > 16384 else max(256, 1 << (total - 1).bit_length())
        dec.setup_caches(1, min(cap, dec.config.block_size), kv_cache_dtype=kv_cache_dtype)
        if dec.lm_head_dtype != lm_head_dtype:  # (the request's head, fp16 without the keyword)
            self._evict("graph")  # (a switch re-allocates the step's buffers: no cached graph survives it, whichever head it was captured under)
            try:
                dec.set_lm_head_dtype(lm_head_dtype)
            except ValueError as e:
                raise ValueError(str(e) if str(e).startswith("lm_head_dtype='int8': ") else "lm_head_dtype='int8': " + str(e)) from None
        key = (self.precision, dec.max_seq_length, dec.kv_cache_dtype, req["temperature"], req["top_k"], req["top_p"], req["repetition_penalty"], req["suppress_tokens"]) \
            + ((("logprobs", True), ) if logprobs else ()) + ((("min_p", req["min_p"]), ) if req["min_p"] else ()) \
            + ((("top_logprobs", top_logprobs), ) if top_logprobs else ()) + ((("lm_head", "int8"), ) if lm_head_dtype == "int8" else ()) \
            + tuple((k, tuple(sorted(v.items())) if isinstance(v, dict) else v.key() if k == "token_fsm" else v) for k, v in sorted((adjust or {}).items()))
        graph = self._native_cache.get(("graph",) + key)
        if graph is None:
            self._evict("graph")
            # (eight token steps per graph replay -- the host looks at the sequence once per `chunk` = 32 tokens anyway; what is left of a
            # chunk runs through the single-step graph over the same state: exactly the steps asked for)
            graph = gen.DecodeGraph(dec, self.device, native_sampling=True, fold_embed=True, seq_capacity=dec.max_seq_length + 1,
                                    seed=self._SAMPLER_SEED, temperature=req["temperature"], top_k=req["top_k"], top_p=req["top_p"], steps_per_replay=8,
                                    repetition_penalty=req["repetition_penalty"], suppress_tokens=req["suppress_tokens"],
                                    **({"logprobs": True} if logprobs else {}), **({"min_p": req["min_p"]} if req["min_p"] else {}),
                                    **({"top_logprobs": top_logprobs} if top_logprobs else {}), **(adjust or {}))
            self._native_cache[("graph",) + key] = graph
        ids32 = ids.view(-1).to(torch.int32)

        def run(n):
            for _ in range(n // graph.steps_per_replay):
                graph.step()
            for _ in range(n % graph.steps_per_replay):
                graph.step_one()
        with torch.inference_mode():
            if T > 1:  # the prompt but for its last token fills the caches (HIP prompt pass; one eager step for a single token)
                pre, pos = ids32[:T - 1], torch.arange(0, T - 1, device=self.device, dtype=torch.int32)
                if dec.prefill_ready(pre):
                    dec.prefill_native(pre, pos, start=0)
                elif T - 1 == 1:
                    dec.decode_native(pre.view(1), pos.view(1))
                else:
                    dec(pre.view(1, -1), pos)
            graph.set_token(ids32[T - 1:T], T - 1)
            return self._run_request(req, ids, graph.sampler, run, chunk, logprobs, top_logprobs)

    # -- route 2: the module tree, decode step captured -------------------------------------------------------------------
    def _generate_captured(self, req, chunk=32):
        """bs = 1 decode on the HF module tree with ONE hipGraph per token: the step `logits = model(input_ids [1,1], StaticCache,
        cache_position)` + the fused sampler (FusedSampler.launch: the draw, EOS suppression, the sequence store, token feedback) are
        captured once per (precision, cache length, sampling) and replayed; the prompt runs eagerly through the same cache."""
        ids, T, max_new = req["ids"].to(self.device), req["T"], req["max_new"]
        total = T + max_new
        key = ("cap", self.precision, total, req["temperature"], req["top_k"], req["top_p"], req["repetition_penalty"], req["suppress_tokens"])
        st = self._native_cache.get(key)
        # (no_grad, not inference_mode: the first graph capture of a process creates the generator's graph-safe state tensors, and
        # inference tensors could not be updated by the captures that follow outside inference mode)
        with torch.no_grad():
            if st is None:
                self._evict("cap")  # (the old entry's graph is destroyed HERE, before the new capture begins)
                st = _CapturedStep(self.model, self.config, self.device, total, req["temperature"], req["top_k"], self._SAMPLER_SEED, req["top_p"],
                                   req["repetition_penalty"], req["suppress_tokens"])
                self._native_cache[key] = st
            st.cache.reset()
            if T > 1:
                self.model(input_ids=ids[:, :T - 1], past_key_values=st.cache, use_cache=True)
            st.tok64.copy_(ids[:, T - 1:T])
            st.tok.copy_(ids.view(-1)[T - 1:T].to(torch.int32))
            st.pos.fill_(T - 1)

            def run(n):
                if st.graph is None:  # (behind the request's set-up: the capture restores the counter word and the prompt's `seen` set)
                    st.capture(T)
                for _ in range(n):
                    st.graph.replay()
            return self._run_request(req, ids, st.sampler, run, chunk)

    @staticmethod
    def _load_config(model_path, trust_remote_code=True):
        from transformers import AutoConfig
        return AutoConfig.from_pretrained(model_path, trust_remote_code=trust_remote_code)

    @classmethod
    def from_config_random(cls, config, precisions=None, device=None, seed=0, torch_dtype=torch.float16):
        """the module tree of `config` (a transformers config with the `anyprec` section) with synthetic weights, no checkpoint"""
        return cls(model_path=None, config=config, precisions=precisions, torch_dtype=torch_dtype, device=device, random_init_seed=seed)

    @classmethod
    def from_quantized(cls, quant_model_path, trust_remote_code=True, fuse_layers=False, precisions=None, local_dir=None,
                       torch_dtype=torch.float16, device=None):
        config = cls._load_config(quant_model_path, trust_remote_code)
        return cls(model_path=quant_model_path, precisions=precisions, config=config, fuse_layers=fuse_layers,
                   trust_remote_code=trust_remote_code, local_dir=local_dir, torch_dtype=torch_dtype, device=device)

    def prune_precisions(self):
        for ap_linear in self.ap_linears:
            ap_linear.prune_precisions()
        gc.collect()

    def set_precision(self, precision):
        for ap_linear in self.ap_linears:
            ap_linear.set_precision(precision)
        self.precision = precision

    def tie_weights(self):
        if hasattr(self.model, "tie_weights"):
            self.model.tie_weights()

    def fuse_layers(self):
        # the reference leaves this a TODO (AnyPrecisionForCausalLM.py:192-196); the fused decode model is `native_decoder`
        raise NotImplementedError("layer fusion inside the HF module tree is not implemented (as in the reference); use "
                                  "native_decoder(bitwidth) for the fused QKV / Up-Gate decode path")

    def native_decoder(self, bitwidth: Optional[int] = None, release_planes: bool = False, kv_cache_dtype=None, lm_head_dtype=None):
        """the same checkpoint as the fused gpt-fast `Transformer` (fused QKV / Up-Gate Any-Precision linears at one precision)
        whose bs=1 decode step runs as the captured 5-launches-per-layer HIP graph.  Built from the module tree's tensors BY
        REFERENCE: embedding, lm_head, norms, o_proj and down_proj are the same storage; q/k/v and gate/up are concatenated into the
        fused tensors layer by layer.
        release_planes=True (what `generate(native=True)` asks for), when the checkpoint carries exactly this precision -- the
        GuidedQuant case: the module tree's own q/k/v/gate/up planes are released as the fused tensors are built (one copy of every
        weight; restored from the fused tensors the first time the module tree is used again through this wrapper, a linear's forward,
        `state_dict()` of the wrapper or of `self.model`, or `.to()` -- `_restore_module_tree`).  The default keeps the module tree whole
        (the fused q/k/v/gate/up tensors are then a second copy: 1.1 GB for an 8B 2-bit model).
        lm_head_dtype ("fp16" / "int8"; None: the decoder's head as it is): the decoder comes back with that head
        (Transformer.set_lm_head_dtype: the int8 copy costs N*K + 4N bytes next to the shared fp16 head)."""
        from .head_q8 import lm_head_dtype_name
        from .model import kv_cache_dtype_name
        hd = None if lm_head_dtype is None else lm_head_dtype_name(lm_head_dtype)
        kv = None if kv_cache_dtype is None else kv_cache_dtype_name(kv_cache_dtype)
        bitwidth = bitwidth or min(self.precisions)
        dec = self._native_cache.get(("decoder", bitwidth))
        if dec is not None and release_planes and not self._released and all(lin.qweight.shape[0] == bitwidth for lin in self.ap_linears):
            self._drop_native()  # (built without the release: built again, releasing as it goes)
            dec = None
        if dec is None:
            self._restore_module_tree()  # (a decoder of another precision may hold the q/k/v/gate/up planes)
            dec = self._build_native(bitwidth, release_planes)
            self._native_cache[("decoder", bitwidth)] = dec
        if kv is not None and (kv != dec.kv_cache_dtype or not dec.cache_initialized):
            # (kv_cache_dtype given: the decoder comes back with caches of that dtype -- the ones it has, re-allocated, or 8 positions)
            if kv == "fp8" and dec.kv8_unserved():
                raise ValueError("kv_cache_dtype='fp8': " + dec.kv8_unserved())
            dec.setup_caches(max(1, dec.max_batch_size), max(8, dec.max_seq_length), kv_cache_dtype=kv)
        if hd is not None and hd != dec.lm_head_dtype:
            dec.set_lm_head_dtype(hd)
        return dec

    def _layer_linears(self, layer):
        at, mlp = layer.self_attn, layer.mlp
        return dict(q=at.q_proj, k=at.k_proj, v=at.v_proj, o=at.o_proj, gate=mlp.gate_proj, up=mlp.up_proj, down=mlp.down_proj)

    def _build_native(self, bitwidth, release_planes=False):
        from .APLinear import APLinear
        from .hf_loader import model_args_from_hf_config
        from .model import Transformer
        if bitwidth not in self.precisions:
            raise ValueError(f"bitwidth {bitwidth} not among the loaded precisions {self.precisions}")
        cfg = self.config.to_dict() if hasattr(self.config, "to_dict") else dict(self.config)
        args = model_args_from_hf_config(cfg, sliding_window=True)
        dev = self.device
        with torch.device("meta"):
            dec = Transformer(torch.float16, args, linear_class=APLinear, linear_kwargs=dict(bitwidth=bitwidth, device="meta"), fuse_linears=True)
        inner = _get_by_path(self.model, (self.config.anyprec.get('arch_config') or {}).get('model_name', 'model'))
        lm_head = self.model.get_output_embeddings() if hasattr(self.model, "get_output_embeddings") else self.model.lm_head
        dec.tok_embeddings.weight = inner.embed_tokens.weight
        dec.output.weight = lm_head.weight
        dec.norm.weight = inner.norm.weight
        # (released only when the planes ARE this precision: nothing is lost by releasing them)
        single = bool(release_planes) and all(lin.qweight.shape[0] == bitwidth for lin in self.ap_linears)

        def put(mod, qweight, lut):
            mod._buffers["qweight"] = qweight
            mod._buffers["lut"] = lut
            mod.output = torch.zeros((1, 1, mod.out_features), dtype=torch.float16, device=dev)

        # what has been released is on record BEFORE the first plane goes (with the decoder that now holds it): a failure at layer k
        # (out of memory in a concatenation, ...) gives layers < k their planes back before the error travels on
        released = []
        if single:
            self._evict("cap")  # (captured steps of the module tree point at the planes about to go)
            self._released = (bitwidth, released, dec)
        restore = _WeakRestore(self)
        try:
            for hf_layer, blk in zip(self.get_model_layers(), dec.layers):
                L = self._layer_linears(hf_layer)
                # (a bias only where the block layout has one: q / k / v of a Qwen2 tree, all three)
                biased = sorted(n for n, m in L.items() if m.bias is not None)
                if biased != (["k", "q", "v"] if args.attn_bias else []):
                    raise NotImplementedError("fused decode model: biased linears (%s)" % ", ".join(biased or ["q / k / v without a bias"]))
                blk.input_layernorm.weight = hf_layer.input_layernorm.weight
                blk.post_attention_layernorm.weight = hf_layer.post_attention_layernorm.weight
                if args.qk_norm:  # (Qwen3: the per-head norms by reference, like the layer norms)
                    blk.attention.q_norm.weight = hf_layer.self_attn.q_norm.weight
                    blk.attention.k_norm.weight = hf_layer.self_attn.k_norm.weight
                lut = lambda m: m._buffers[f"lut{bitwidth}"].to(torch.float16)  # noqa: E731
                put(blk.attention.wo, L["o"].qweight[:bitwidth], lut(L["o"]))           # (a prefix of the planes: contiguous view)
                put(blk.feed_forward.w2, L["down"].qweight[:bitwidth], lut(L["down"]))
                put(blk.attention.wqkv, torch.cat([L[n].qweight[:bitwidth] for n in "qkv"], dim=1).contiguous(),
                    torch.cat([lut(L[n]) for n in "qkv"], dim=0).contiguous())
                put(blk.feed_forward.w1w3, torch.cat([L["gate"].qweight[:bitwidth], L["up"].qweight[:bitwidth]], dim=1).contiguous(),
                    torch.cat([lut(L["gate"]), lut(L["up"])], dim=0).contiguous())
                if args.attn_bias:  # (a new tensor, like the concatenated planes; the module tree keeps its own three)
                    blk.attention.wqkv._buffers["bias"] = torch.cat([L[n].bias.to(torch.float16) for n in "qkv"], dim=0).contiguous()
                if single:
                    released.append(hf_layer)
                    for n in ("q", "k", "v", "gate", "up"):
                        L[n]._buffers["qweight"] = torch.empty((0, ), dtype=torch.int32, device=dev)
                        L[n]._gq_restore = restore
            dec = dec.eval()
            dec._reset_native()
        except BaseException:
            self._restore_module_tree()
            raise
        if not released:
            self._released = None
        return dec

    def _drop_native(self):
        self._restore_module_tree()
        self._evict("graph")
        self._evict("cap")
        self._native_cache = {}

    def _apply(self, fn, *args, **kwargs):
        # .to() / .half() / .cuda(): the module tree gets new tensors -- it takes its planes back first, and the fused decode model (built
        # over the old tensors by reference) and every captured graph are stale
        if getattr(self, "_native_cache", None) is not None:
            self._drop_native()
        return super()._apply(fn, *args, **kwargs)

    def _restore_module_tree(self):
        """give q/k/v and gate/up of the module tree their plane tensors back (slices of the fused decode model's tensors; the gate/up
        rows un-paired), and drop the fused model and its graphs -- one copy of every weight at any time.  Works from its own record
        (`_released` = precision, the layers released so far, the decoder holding their planes), not from the cache."""
        rel = getattr(self, "_released", None)
        if not rel:
            return
        from .model import _pair_perm
        bitwidth, layers, dec = rel
        self._released = None
        done = {id(l) for l in layers}
        for hf_layer, blk in zip(self.get_model_layers(), dec.layers):
            if id(hf_layer) not in done:
                continue
            L = self._layer_linears(hf_layer)
            qkv, gu = blk.attention.wqkv.qweight, blk.feed_forward.w1w3.qweight
            if getattr(blk.feed_forward.w1w3, "gq_row_pairs", False):
                gu = gu[:, torch.argsort(_pair_perm(gu.shape[1] // 2, gu.device)), :]
            r0 = 0
            for n in ("q", "k", "v"):
                L[n]._buffers["qweight"] = qkv[:, r0:r0 + L[n].out_features, :].contiguous()
                r0 += L[n].out_features
            L["gate"]._buffers["qweight"] = gu[:, :L["gate"].out_features, :].contiguous()
            L["up"]._buffers["qweight"] = gu[:, L["gate"].out_features:, :].contiguous()
            for n in ("q", "k", "v", "gate", "up"):
                L[n]._gq_restore = None
            blk.attention.wqkv._buffers["qweight"] = blk.feed_forward.w1w3._buffers["qweight"] = None
        self._evict("graph")
        self._evict("cap")
        self._native_cache = {k: v for k, v in self._native_cache.items() if k[0] != "decoder"}
        gc.collect()
