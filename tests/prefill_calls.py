"""What one eager prompt pass (`Transformer.prefill_native` / `score_native`) asks of the C ABI, as a log that two commits can be compared by.

The recorder and the pointer roles are tests/decode_calls.py's (`Recorder`, `regions_of`): every call in order with its entry point, its
scalars as they are and every pointer as a role -- a parameter or buffer by module path (the KV caches and their scales among them), the
RoPE tables, `null`, or `anon` for the pass's transients (the embedded rows, the chunk buffers, the linears' outputs and workspaces).
The linears' own launches (gq_anyprec_gemm_ws, gq_anyprec_gemv, gq_qtip_gemm_ws, ..) and the host queries (gq_attn_prefill_supported,
gq_head_nll_ws_bytes) are part of the log.  What the pass does outside the library -- SDPA, the torch heads -- shows in the last entry,
`["result", [last_prefill_plan, output shapes]]`.

`CONFIGS` are two-layer models of tests/test_prefill_chunked_gpu.py's builders (dim 512, 8 / 2 heads, head_dim 64, vocab 1024) and one
QTIP model of decode_calls', a cache of 80 rows, 17 tokens, whole or in chunks of 16: the pieces (0, 16) and (16, 1), a one-token tail.
`COVERAGE` names the branch every configuration is there for.  tools/record_prefill_calls.py writes the log of a commit to
tests/golden/prefill_calls.json (and refuses to when a branch is missing), tests/test_prefill_calls_golden_gpu.py compares for equality.
"""
import os

import decode_calls
from decode_calls import _args, _names, _roles

KNOBS = decode_calls.KNOBS + ("GQ_PREFILL_ATTN", "GQ_PREFILL_CHUNK", "GQ_SCORE_HEAD")
CACHE, S, CHUNK = 80, 17, 16

# name -> (model, KV cache dtype, call, chunk, last_only, knobs)
CONFIGS = {
    "llama_whole": ("llama-2bit", "fp16", "prefill", None, False, {}),
    "llama_chunked": ("llama-2bit", "fp16", "prefill", CHUNK, False, {}),
    "llama_chunked_last_only": ("llama-2bit", "fp16", "prefill", CHUNK, True, {}),
    "llama_chunked_sdpa": ("llama-2bit", "fp16", "prefill", CHUNK, False, {"GQ_PREFILL_ATTN": "0"}),
    "qwen3_chunked": ("qwen3", "fp16", "prefill", CHUNK, False, {}),
    "qwen2_chunked": ("qwen2", "fp16", "prefill", CHUNK, False, {}),
    "window24_chunked": ("window24", "fp16", "prefill", CHUNK, False, {}),
    "llama_kv8": ("llama-2bit", "fp8", "prefill", CHUNK, False, {}),
    "qwen3_kv8": ("qwen3", "fp8", "prefill", CHUNK, False, {}),
    "qwen2_kv8": ("qwen2", "fp8", "prefill", CHUNK, False, {}),
    "llama_kv8_sdpa": ("llama-2bit", "fp8", "prefill", CHUNK, False, {"GQ_PREFILL_ATTN": "0"}),
    "qtip_chunked": ("qtip", "fp16", "prefill", CHUNK, False, {}),
    "llama_score_kernel": ("llama-2bit", "fp16", "score", CHUNK, False, {"GQ_SCORE_HEAD": "1"}),
    "llama_score_torch": ("llama-2bit", "fp16", "score", CHUNK, False, {"GQ_SCORE_HEAD": "0"}),
}

_models = {}


def _model(kind, kv):
    """one model per kind for the process; its caches follow the configuration (a change of the dtype re-allocates them)"""
    import torch
    if kind not in _models:
        if kind == "qtip":
            _models[kind] = decode_calls._build("qtip", 2, decode_calls.QSMALL, CACHE)
        else:
            import test_prefill_chunked_gpu
            _models[kind] = test_prefill_chunked_gpu._BUILD[kind]()
    m = _models[kind]
    with torch.device("cuda:0"):
        m.setup_caches(1, CACHE, kv_cache_dtype=kv)
    return m


def record(name):
    """the calls of one eager prompt pass of configuration `name`, and what it reported"""
    import torch
    from guidedquant_amd import _lib
    kind, kv, what, chunk, last_only, knobs = CONFIGS[name]
    L = _lib.lib()
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        os.environ.update(knobs)
        L.gq_reset_env_cache()
        _lib.check(L.gq_set_ap_mode(0), "gq_set_ap_mode")
        m = _model(kind, kv)
        assert m.kv_cache_dtype == kv and m._native_kind() == ("qtip" if kind == "qtip" else "ap"), (name, m._native_kind())
        d = torch.device("cuda:0")
        g = torch.Generator(device=d).manual_seed(S)
        idx = torch.randint(0, m.config.vocab_size, (1, S), dtype=torch.int32, device=d, generator=g)
        pos = torch.arange(S, dtype=torch.int32, device=d)

        def run():
            with torch.no_grad():
                if what == "score":
                    return m.score_native(idx, chunk=chunk)
                return (m.prefill_native(idx, pos, start=0, last_only=last_only, chunk=chunk), )
        assert m.prefill_ready(idx)
        m._native_state()
        run()  # (whatever a linear sets up on its first rows happens here, not inside the log)
        torch.cuda.synchronize()
        rec = decode_calls.Recorder(L, decode_calls.regions_of(m))
        _lib._lib = rec
        try:
            out = run()
            torch.cuda.synchronize()
        finally:
            _lib._lib = L
        assert all(bool(torch.isfinite(o.float()).all()) for o in out), name
        plan = m.last_prefill_plan
        result = dict(chunks=[list(c) for c in plan["chunks"]], attn=list(plan["attn"]), head=plan.get("head"), out=[list(o.shape) for o in out])
        return rec.calls + [["result", [result]]]
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(saved)
        L.gq_reset_env_cache()
        L.gq_set_ap_mode(-1)


# ------------------------------------------------------------------------------------------------ coverage
ATTN = ("gq_attn_prefill", "gq_attn_prefill_kv8")
ROWS = ("gq_rope_cache_rows", "gq_qknorm_rope_cache_rows", "gq_rope_cache_rows_kv8")
V = 1024


def _result(calls):
    assert calls[-1][0] == "result"
    return calls[-1][1][0]


def _only_rows(calls, entry):
    """every row write of the log goes through `entry`: twice per piece (two layers, two pieces unless the pass is whole)"""
    n = [len(_args(calls, e)) for e in ROWS]
    return n[ROWS.index(entry)] == 2 * len(_result(calls)["chunks"]) and sum(n) == n[ROWS.index(entry)]


def _no_bias_role(calls):
    return not any("bias" in r for r in _roles(calls))


def _kv8(norm):
    def pred(c):
        a = _args(c, "gq_rope_cache_rows_kv8")
        want = [(f"layers.{i}.attention.q_norm.weight+0", f"layers.{i}.attention.k_norm.weight+0") if norm else ("null", "null") for i in (0, 1)] * 2
        return (_only_rows(c, "gq_rope_cache_rows_kv8") and [(x[14], x[15]) for x in a] == want and all(x[17] == "null" for x in a)
                and all(x[7].endswith("kv_cache.k_inv+0") and x[8].endswith("kv_cache.v_inv+0") for x in a)
                and [x[7] for x in _args(c, "gq_attn_prefill_kv8")] == [0, 0, 16, 16] and "gq_attn_prefill" not in _names(c)
                and _result(c)["attn"] == ["hip-kv8"] * 2)
    return pred


# (branch, configuration, what its log must show)
COVERAGE = [
    ("llama, one piece, auto: SDPA, no gq_attn_prefill", "llama_whole",
     lambda c: not any(n in _names(c) for n in ATTN) and _only_rows(c, "gq_rope_cache_rows") and _result(c)["chunks"] == [[0, 17]]
     and _result(c)["attn"] == ["sdpa"] * 2 and _result(c)["out"] == [[1, 17, V]]),
    ("llama chunked, auto: gq_attn_prefill with start 0 and 16", "llama_chunked",
     lambda c: [(a[4], a[5], a[11]) for a in _args(c, "gq_attn_prefill")] == [(16, 0, 0)] * 2 + [(1, 16, 0)] * 2
     and _result(c)["chunks"] == [[0, 16], [16, 1]] and _result(c)["attn"] == ["hip"] * 2 and _only_rows(c, "gq_rope_cache_rows")),
    ("GQ_PREFILL_ATTN=0 chunked: SDPA", "llama_chunked_sdpa",
     lambda c: not any(n in _names(c) for n in ATTN) and _result(c)["chunks"] == [[0, 16], [16, 1]] and _result(c)["attn"] == ["sdpa"] * 2),
    ("qwen3: gq_qknorm_rope_cache_rows with the q_norm / k_norm weights of its layer", "qwen3_chunked",
     lambda c: _only_rows(c, "gq_qknorm_rope_cache_rows") and [(a[12], a[13]) for a in _args(c, "gq_qknorm_rope_cache_rows")]
     == [(f"layers.{i}.attention.q_norm.weight+0", f"layers.{i}.attention.k_norm.weight+0") for i in (0, 1)] * 2),
    ("qwen2: gq_rope_cache_rows, no bias pointer anywhere (the linears add it)", "qwen2_chunked",
     lambda c: _only_rows(c, "gq_rope_cache_rows") and _no_bias_role(c)),
    ("layer_windows=(None, 24): window 0 then 24", "window24_chunked", lambda c: [a[11] for a in _args(c, "gq_attn_prefill")] == [0, 24, 0, 24]),
    ("fp8 cache, llama: gq_rope_cache_rows_kv8 without norm or bias + gq_attn_prefill_kv8", "llama_kv8", _kv8(False)),
    ("fp8 cache, qwen3: the norm weights ride in gq_rope_cache_rows_kv8", "qwen3_kv8", _kv8(True)),
    ("fp8 cache, qwen2: a null bias (the linears added it)", "qwen2_kv8", lambda c: _kv8(False)(c) and _no_bias_role(c)),
    ("fp8 cache, GQ_PREFILL_ATTN=0: no prefill attention entry", "llama_kv8_sdpa",
     lambda c: not any(n in _names(c) for n in ATTN) and _only_rows(c, "gq_rope_cache_rows_kv8") and _result(c)["attn"] == ["sdpa-kv8"] * 2),
    ("QTIP: gate | up side by side, paired = 0 in gq_silu_mul_rows", "qtip_chunked",
     lambda c: [a[4] for a in _args(c, "gq_silu_mul_rows")] == [0] * 4 and _only_rows(c, "gq_rope_cache_rows")),
    ("AP: the paired gate / up rows of the decode step, paired = 1", "llama_chunked", lambda c: [a[4] for a in _args(c, "gq_silu_mul_rows")] == [1] * 4),
    ("score_native chunked, GQ_SCORE_HEAD=1: gq_head_nll_ws_bytes + gq_head_nll once per piece", "llama_score_kernel",
     lambda c: [n for n in _names(c) if n.startswith("gq_head_nll")] == ["gq_head_nll_ws_bytes", "gq_head_nll"] * 2
     and [a[3] for a in _args(c, "gq_head_nll")] == [16, 1] and _result(c)["head"] == "hip-nll" and _result(c)["out"] == [[16], [16]]),
    ("score_native chunked, GQ_SCORE_HEAD=0: neither", "llama_score_torch",
     lambda c: not any(n.startswith("gq_head_nll") for n in _names(c)) and _result(c)["head"] == "torch" and _result(c)["out"] == [[16], [16]]),
]


def missing_coverage(logs):
    """the branches of COVERAGE a set of logs does not show"""
    missing = [what for what, name, pred in COVERAGE if not pred(logs[name])]
    # last_only=True chunked: the same launches as the pass with every row's logits, the head on the last piece's last row only
    a, b = logs["llama_chunked_last_only"], logs["llama_chunked"]
    if not (a[:-1] == b[:-1] and _result(a)["out"] == [[1, 1, V]] and _result(b)["out"] == [[1, 17, V]] and _result(a)["chunks"] == _result(b)["chunks"]):
        missing.append("last_only=True chunked: the launches of last_only=False, one row of logits")
    return missing
