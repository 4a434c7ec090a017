"""LoRA adapters beside the quantized base: the host side of gq_lora_down / gq_lora_up (csrc/lora.hip, include/gq_hip.h).

A 2- to 8-bit Any-Precision weight is a per-row codebook index, so `W + s B A` cannot be merged into it: the adapter runs next to the base
at inference time.  The fused decode step (native_step.ApStep.layers) serves three sites per layer:

    qkv    x -> RMSNorm -> A -> B, rows laid out like the packed q | k | v vector: the `qkv_bias` of gq_attn_decode_split_bias
    o      the attention output y -> A -> B, added to the residual the wo launch takes
    down   the silu(gate) * up vector -> A -> B, added to the residual the w2 launch takes

`LoraAdapter.from_peft` reads peft's key layout and adapter_config.json fields; `bind` (called by `Transformer.set_adapter`) checks the
shapes against the model and stacks the matrices of a site into the tensors the kernels read: A [R][K] with every rank padded to a multiple
of 16 by zero rows, B one run of [rows][padded rank] per segment, and the GqLoraSeg table.  The prompt pass applies the same deltas per row
with torch matmuls (`LoraSite.delta_rows`).
"""
import json
import os
import re

import torch

from . import _lib

MAX_RANK = 64
SITES = ("qkv", "o", "down")
_KEY = re.compile(r"layers\.(\d+)\.(?:self_attn|mlp)\.([a-z]+_proj)\.lora_([AB])(?:\.[A-Za-z0-9_]+)?\.weight$")
_SERVED = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")


def _pad16(r):
    return (r + 15) // 16 * 16


def _pattern(patterns, path, default):
    """peft's rank_pattern / alpha_pattern: the value of the first key that is the module path or a suffix of it (as a regular expression)"""
    for key, val in (patterns or {}).items():
        if key == path or re.match(rf"(.*\.)?({key})$", path):
            return val
    return default


class LoraSite:
    """one site of one layer on the device: what the two launches and the prompt pass read"""

    def __init__(self, parts, N, K, device):
        """parts: [(row_begin, row_end, A fp32 [r, K], B fp32 [rows, r], scale)] ascending in rows"""
        self.N, self.K = N, K
        ranks = [_pad16(a.shape[0]) for _, _, a, _, _ in parts]
        self.R = sum(ranks)
        A = torch.zeros(self.R, K, dtype=torch.float16)
        Bs, segs, t0, b0 = [], [], 0, 0
        for (rb, re_, a, b, s), rp in zip(parts, ranks):
            r = a.shape[0]
            A[t0:t0 + r] = a.to(torch.float16)
            bp = torch.zeros(re_ - rb, rp, dtype=torch.float16)
            bp[:, :r] = b.to(torch.float16)
            Bs.append(bp.reshape(-1))
            segs.append((rb, re_, t0, rp, b0, float(s)))
            t0, b0 = t0 + rp, b0 + bp.numel()
        self.segments = segs
        self.A = A.to(device).contiguous()
        self.B = torch.cat(Bs).to(device).contiguous()
        self.seg_array = (_lib.GqLoraSeg * len(segs))(*[_lib.GqLoraSeg(*s) for s in segs])

    def launch(self, L, x, norm_weight, eps, partials, base, out, stream):
        """the site's two launches: x (and the RMSNorm weight of the qkv site) -> partials -> out = base + delta"""
        n = L.gq_lora_n_partials(self.K)
        _lib.check(L.gq_lora_down(x, norm_weight, eps, self.A.data_ptr(), self.R, self.K, partials, stream), "gq_lora_down")
        _lib.check(L.gq_lora_up(partials, n, self.R, self.B.data_ptr(), self.seg_array, len(self.segments), base, out, self.N, stream), "gq_lora_up")

    def delta_rows(self, xh):
        """the prompt pass: fp16 [S, N] = fp16(s (xh A^T) B^T) per segment for the rows xh fp16 [S, K], zero where no segment lies"""
        S = xh.shape[0]
        out = torch.zeros(S, self.N, dtype=torch.float16, device=xh.device)
        xf = xh.float()
        for rb, re_, t0, rp, b0, s in self.segments:
            t = xf @ self.A[t0:t0 + rp].float().T
            out[:, rb:re_] = (s * (t @ self.B[b0:b0 + (re_ - rb) * rp].view(re_ - rb, rp).float().T)).to(torch.float16)
        return out


class LoraAdapter:
    """`modules[(layer, name)] = (A fp32 [r, in], B fp32 [out, r], scale)` as parsed; `layers[i][site]` = LoraSite | None once bound"""

    def __init__(self, modules):
        self.modules = modules
        self._bindings = {}  # (geometry, device) -> the sites per layer: every model an adapter serves keeps its own
        self.layers = None   # the binding made last

    @classmethod
    def from_peft(cls, state_dict, config, model_config=None, device=None):
        """state_dict: peft's `...layers.{i}.self_attn.{q,k,v,o}_proj.lora_{A,B}.weight` / `...mlp.down_proj...` keys (an adapter name behind
        lora_A / lora_B is accepted); config: the fields of adapter_config.json.  With model_config (ModelArgs) the adapter is bound at once."""
        cfg = dict(config)
        # peft's three forms of target_modules: a list of module names (suffixes), "all-linear", or one regular expression for the
        # whole module path -- the last two say nothing a key does not, so the keys decide
        targets = cfg.get("target_modules") or []
        target_re = targets if isinstance(targets, str) and targets != "all-linear" else None
        targets = [] if isinstance(targets, str) else list(targets)
        bad = sorted(t for t in targets if t.split(".")[-1] in ("gate_proj", "up_proj"))
        if bad:
            raise ValueError(f"lora: target {', '.join(bad)}: a gate / up delta belongs in front of SiLU, inside the w1w3 launch (not served)")
        if cfg.get("use_dora"):
            raise ValueError("lora: use_dora is not served")
        if cfg.get("use_rslora"):
            raise ValueError("lora: use_rslora=True is not served (scaling is lora_alpha / r)")
        if cfg.get("bias", "none") != "none":
            raise ValueError(f"lora: bias={cfg['bias']!r} is not served (adapter biases)")
        if cfg.get("modules_to_save"):
            raise ValueError("lora: modules_to_save is not served")
        if "r" not in cfg or "lora_alpha" not in cfg:
            raise ValueError("lora: the adapter config needs r and lora_alpha")
        found = {}
        for key, t in state_dict.items():
            m = _KEY.search(key)
            if m is None:
                raise ValueError(f"lora: unexpected key {key!r}")
            layer, name, ab = int(m.group(1)), m.group(2), m.group(3)
            if name not in _SERVED:
                raise ValueError(f"lora: target {name} (key {key!r}) is not served" + (": a gate / up delta belongs in front of SiLU, inside the "
                                                                                       "w1w3 launch" if name in ("gate_proj", "up_proj") else ""))
            path = key[:m.start()] + f"layers.{layer}." + ("mlp." if name == "down_proj" else "self_attn.") + name
            if targets and name not in [t_.split(".")[-1] for t_ in targets]:
                raise ValueError(f"lora: key {key!r} is not among target_modules {targets}")
            if target_re and not any(re.fullmatch(target_re, q) for q in (path, path.removeprefix("base_model.model."))):
                raise ValueError(f"lora: key {key!r} does not match target_modules {target_re!r}")
            found.setdefault((layer, name), {"path": path})[ab] = torch.as_tensor(t).detach().to("cpu", torch.float32)
        modules = {}
        for (layer, name), d in sorted(found.items()):
            if "A" not in d or "B" not in d:
                raise ValueError(f"lora: layer {layer} {name}: lora_A and lora_B come in pairs")
            A, B = d["A"], d["B"]
            r = int(_pattern(cfg.get("rank_pattern"), d["path"], cfg["r"]))
            alpha = float(_pattern(cfg.get("alpha_pattern"), d["path"], cfg["lora_alpha"]))
            if r > MAX_RANK:
                raise ValueError(f"lora: layer {layer} {name}: rank {r} above {MAX_RANK}")
            if A.dim() != 2 or B.dim() != 2 or r < 1 or A.shape[0] != r or B.shape[1] != r:
                raise ValueError(f"lora: layer {layer} {name}: shapes {tuple(A.shape)} / {tuple(B.shape)} do not match rank {r}")
            modules[(layer, name)] = (A, B, alpha / r)
        if not modules:
            raise ValueError("lora: the adapter holds no lora_A / lora_B weights")
        ad = cls(modules)
        if model_config is not None:
            ad.bind(model_config, device or "cpu")
        return ad

    @classmethod
    def from_dir(cls, path, model_config=None, device=None):
        """a peft adapter directory: adapter_config.json + adapter_model.bin (torch.load), or adapter_model.safetensors where the
        safetensors package is importable"""
        with open(os.path.join(path, "adapter_config.json")) as f:
            cfg = json.load(f)
        bin_path, st_path = os.path.join(path, "adapter_model.bin"), os.path.join(path, "adapter_model.safetensors")
        if os.path.exists(bin_path):
            sd = torch.load(bin_path, map_location="cpu", weights_only=True)
        elif os.path.exists(st_path):
            try:
                from safetensors.torch import load_file
            except ImportError:
                raise ValueError(f"lora: {st_path} needs the safetensors package; save the adapter as adapter_model.bin") from None
            sd = load_file(st_path)
        else:
            raise ValueError(f"lora: no adapter_model.bin or adapter_model.safetensors in {path}")
        return cls.from_peft(sd, cfg, model_config, device)

    def targets(self, site):
        names = dict(qkv=("q_proj", "k_proj", "v_proj"), o=("o_proj", ), down=("down_proj", ))[site]
        return any(n in names for _, n in self.modules)

    def bind(self, c, device):
        """check every shape against the model (ModelArgs) and build the device tensors: the sites per layer, `[i][site]` = LoraSite | None
        (kept per geometry and device); ValueError("lora: ...") on a mismatch"""
        key = (c.n_layer, c.dim, c.n_head, c.n_local_heads, c.head_dim, c.intermediate_size, str(device))
        if key in self._bindings:
            self.layers = self._bindings[key]
            return self.layers
        nq, nkv = c.n_head * c.head_dim, c.n_local_heads * c.head_dim
        geo = dict(q_proj=(nq, c.dim, 0), k_proj=(nkv, c.dim, nq), v_proj=(nkv, c.dim, nq + nkv), o_proj=(c.dim, nq, 0),
                   down_proj=(c.dim, c.intermediate_size, 0))
        layers = [dict.fromkeys(SITES) for _ in range(c.n_layer)]
        parts = {}
        for (layer, name), (A, B, s) in self.modules.items():
            if layer >= c.n_layer:
                raise ValueError(f"lora: layer {layer} of an adapter on a model of {c.n_layer} layers")
            n_out, n_in, row0 = geo[name]
            if tuple(A.shape) != (A.shape[0], n_in) or tuple(B.shape) != (n_out, A.shape[0]):
                raise ValueError(f"lora: layer {layer} {name}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not match the model's "
                                 f"[{n_out}, {n_in}] linear")
            if n_in % 64:
                raise ValueError(f"lora: layer {layer} {name}: input width {n_in} is not a multiple of 64")
            site = "qkv" if name in ("q_proj", "k_proj", "v_proj") else ("o" if name == "o_proj" else "down")
            parts.setdefault((layer, site), []).append((row0, row0 + n_out, A, B, s))
        for (layer, site), p in parts.items():
            N, K = ((nq + 2 * nkv, c.dim) if site == "qkv" else geo["o_proj" if site == "o" else "down_proj"][:2])
            layers[layer][site] = LoraSite(sorted(p, key=lambda e: e[0]), N, K, device)
        self.layers = self._bindings[key] = layers
        return layers
