"""What one eager `Transformer.decode_native` step asks of the C ABI, as a log that two commits can be compared by.

`Recorder` stands in for the ctypes library object (`_lib._lib`) during the step and notes every call in order: the entry point, every
scalar argument as it is, every pointer argument as a ROLE -- `name+byte offset` when it falls inside a registered tensor (the step's
state buffers, the rows of `y32` / `xs16` / `xt`, every parameter and buffer by module path -- the KV caches among them --, the RoPE
tables), `null` for None, `anon` for anything else (the fp32 copies and ctypes arrays the QTIP plans keep).  Descriptor arrays
(GqQtipIn / Out / Xf / Mid, arrays of pointers) are expanded field by field the same way.  The state is built before the recorder goes
in, so the log is the step alone: its launches and the host queries it makes on the way (gq_anyprec_handover_plan, the *_supported
checks).

`CONFIGS` are the models and knob settings of the existing decode tests, cut to two layers; `COVERAGE` names the branch every one of
them is there for.  tools/record_decode_calls.py writes the log of a commit to tests/golden/decode_calls.json (and refuses to when a
branch is missing from it), tests/test_decode_calls_golden_gpu.py replays the configurations and compares for equality.
"""
import bisect
import ctypes
import os
import tempfile

KNOBS = ("GQ_NATIVE_QTIP", "GQ_ATTN_GQA", "GQ_ATTN_SPLIT", "GQ_NATIVE_PAIRS", "GQ_SSQ_HANDOVER", "GQ_QTIP_KSPLIT", "GQ_QTIP_KSPLIT_GROUP",
         "GQ_QTIP_FOLD", "GQ_QTIP_ONE_LAUNCH", "GQ_QTIP_OUT_SEG", "GQ_QTIP_MLP_MID", "GQ_QTIP_ATTN_FOLD", "GQ_QTIP_PRE",
         "GQ_QKV_ATTN", "GQ_PL_MIN_MWEIGHTS", "GQ_ST_KSPLIT", "GQ_HADAMARD_TABLES")
STATE_KEYS = ("x", "h", "y", "qkv", "ssq", "attn_flags", "gu", "logits", "attn_ws", "ap_ws", "g", "u", "y32", "xs16", "xt", "z32")

SMALL = dict(dim=512, n_head=4, n_local_heads=2, intermediate_size=1024, vocab_size=384)       # (the lm_head takes K % 512 == 0)
W8B = dict(dim=4096, n_head=32, n_local_heads=8, intermediate_size=2048, vocab_size=512)       # the 8B attention geometry
QSMALL = dict(dim=512, n_head=4, n_local_heads=4, intermediate_size=1024, vocab_size=384)
Q4096 = dict(dim=4096, n_head=32, n_local_heads=8, intermediate_size=4096, vocab_size=384)       # the planner splits K of wo and down
QWIDE = dict(dim=8192, n_head=64, n_local_heads=8, intermediate_size=4096, vocab_size=384)       # ... and of the q / k / v group
QFACTOR = dict(dim=1024, n_head=8, n_local_heads=8, intermediate_size=11008, vocab_size=384)   # 11008 = 172 * 64 (Llama-2-7b's MLP)

# name -> (family, bits, ModelArgs fields, cache length, knobs)
CONFIGS = {
    "ap4": ("ap", 4, SMALL, 64, {}),
    "ap6_no_pairs": ("ap", 6, SMALL, 64, {"GQ_NATIVE_PAIRS": "0"}),
    "ap2_8b_qkv_rope": ("ap", 2, W8B, 64, {"GQ_PL_MIN_MWEIGHTS": "0"}),
    "ap2_8b_qkv_attn": ("ap", 2, W8B, 64, {"GQ_PL_MIN_MWEIGHTS": "0", "GQ_QKV_ATTN": "1"}),
    "ap2_8b_handover": ("ap", 2, dict(W8B, intermediate_size=14336), 64, {"GQ_SSQ_HANDOVER": "1"}),
    "ap2_8b_long_cache": ("ap", 2, W8B, 2048, {"GQ_PL_MIN_MWEIGHTS": "0"}),
    "ap2_8b_long_cache_no_gqa": ("ap", 2, W8B, 2048, {"GQ_PL_MIN_MWEIGHTS": "0", "GQ_ATTN_GQA": "0"}),
    "ap4_long_cache": ("ap", 4, SMALL, 1100, {}),
    "ap4_attn_split_knob": ("ap", 4, SMALL, 64, {"GQ_ATTN_SPLIT": "2"}),
    "ap4_qk_norm": ("ap", 4, dict(SMALL, qk_norm=True, head_dim=128, norm_eps=1e-6), 64, {}),
    "ap2_down_workspace": ("ap", 2, dict(dim=2048, n_head=16, n_local_heads=4, intermediate_size=18432, vocab_size=512), 32, {}),
    "qtip_pow2": ("qtip", 2, QSMALL, 64, {}),
    "qtip_pow2_4096": ("qtip", 2, Q4096, 64, {}),
    "qtip_pow2_wide": ("qtip", 2, QWIDE, 64, {}),
    "qtip_factor_mlp_mid": ("qtip", 2, QFACTOR, 64, {"GQ_QTIP_MLP_MID": "1"}),
    "qtip_factor_no_mlp_mid": ("qtip", 2, QFACTOR, 64, {"GQ_QTIP_MLP_MID": "0"}),
    "qtip_no_attn_fold": ("qtip", 2, QSMALL, 64, {"GQ_QTIP_ATTN_FOLD": "0"}),
    "qtip_no_out_seg": ("qtip", 2, QSMALL, 64, {"GQ_QTIP_OUT_SEG": "0"}),
    "qtip_no_ksplit": ("qtip", 2, Q4096, 64, {"GQ_QTIP_KSPLIT": "0"}),
    "qtip_no_ksplit_wide": ("qtip", 2, QWIDE, 64, {"GQ_QTIP_KSPLIT": "0"}),
    "qtip_no_ksplit_group": ("qtip", 2, QWIDE, 64, {"GQ_QTIP_KSPLIT_GROUP": "0"}),
    "qtip_fold": ("qtip", 2, QSMALL, 64, {"GQ_QTIP_FOLD": "1"}),
    "qtip_one_launch": ("qtip", 2, QSMALL, 64, {"GQ_QTIP_ONE_LAUNCH": "1"}),
    "qtip_pre": ("qtip", 2, QSMALL, 64, {"GQ_QTIP_PRE": "1"}),
    "qtip_long_cache": ("qtip", 2, QSMALL, 1100, {}),
}


class Recorder:
    """the ctypes library with every call logged as [entry point, [argument, ..]]"""

    def __init__(self, real, regions):
        self._real = real
        self._regions = sorted(regions)  # (start, end, name)
        self._starts = [r[0] for r in self._regions]
        self.calls = []

    def role(self, p):
        if not p:
            return "null"
        i = bisect.bisect_right(self._starts, p) - 1
        if i >= 0 and p < self._regions[i][1]:
            return f"{self._regions[i][2]}+{p - self._regions[i][0]}"
        return "anon"

    def _element(self, e):
        if isinstance(e, ctypes.Structure):
            return {f: (self.role(getattr(e, f)) if t is ctypes.c_void_p else int(getattr(e, f))) for f, t in e._fields_}
        return e

    def _arg(self, t, a):
        if t is ctypes.c_void_p:
            return self.role(a.value if isinstance(a, ctypes.c_void_p) else a)
        if isinstance(t, type) and issubclass(t, ctypes._Pointer):
            if a is None:
                return "null"
            items = [a] if isinstance(a, ctypes.Structure) else ([a.contents] if isinstance(a, ctypes._Pointer) else list(a))
            if t._type_ is ctypes.c_void_p:
                return [self.role(e) for e in items]
            return [self._element(e) for e in items]
        return a

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        types = getattr(fn, "argtypes", None) or []

        def call(*args):
            self.calls.append([name, [self._arg(t, a) for t, a in zip(types, args)]])
            return fn(*args)
        return call


def regions_of(model):
    """(start, end, name) of every registered tensor; taken after the state is built (the gate / up pairing assigns new tensors)"""
    out = []

    def add(name, t):
        if t is not None and hasattr(t, "is_cuda") and t.is_cuda and t.numel():
            out.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name))
    st = model._native_state()
    for k in STATE_KEYS:
        try:
            t = st[k]
        except (KeyError, AttributeError):
            continue
        if t is not None and t.dim() == 2:
            for i in range(t.shape[0]):
                add(f"{k}[{i}]", t[i])
        else:
            add(k, t)
    for name, t in list(model.named_parameters()) + list(model.named_buffers()):
        add(name, t)
    add("rope_cos", model.rope_cos)
    add("rope_sin", model.rope_sin)
    return out


def _build(family, bits, shape, cache):
    import torch
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    name = "decode-calls-" + family
    gm.transformer_configs[name] = dict(dict(model_name="qwen3-llama-decode-calls", block_size=2048, n_layer=2, rope_base=500000), **shape)
    try:
        m = load_model(name, "cuda:0", family, bits, random_init=True)
    finally:
        del gm.transformer_configs[name]
    with torch.device("cuda:0"):
        m.setup_caches(max_batch_size=1, max_seq_length=cache)
    return m


def record(name):
    """the calls of one eager decode step of configuration `name`"""
    import numpy as np
    import torch
    from guidedquant_amd import _lib, qtip
    family, bits, shape, cache, knobs = CONFIGS[name]
    L = _lib.lib()
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    tmp = tempfile.TemporaryDirectory()
    try:
        os.environ.update(knobs)
        if shape["intermediate_size"] == 11008:  # the factor table comes from the caller: the golden fixture's copy
            g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "had_n11008.npz"))
            np.savez(os.path.join(tmp.name, "tables.npz"), had172=g["hadK"])
            os.environ["GQ_HADAMARD_TABLES"] = os.path.join(tmp.name, "tables.npz")
        qtip._tables = None
        L.gq_reset_env_cache()
        _lib.check(L.gq_set_ap_mode(0), "gq_set_ap_mode")
        m = _build(family, bits, shape, cache)
        assert m._native_kind() == family, (name, m._native_kind())
        tok = torch.tensor([5], dtype=torch.int32, device="cuda:0")
        pos = torch.tensor([3], dtype=torch.int32, device="cuda:0")
        m._native_state()
        _lib.current_stream_ptr()  # (the one-time self-check of the library runs here, not inside the log)
        rec = Recorder(L, regions_of(m))
        _lib._lib = rec
        try:
            with torch.no_grad():
                logits = m.decode_native(tok, pos)
            torch.cuda.synchronize()
        finally:
            _lib._lib = L
        assert bool(torch.isfinite(logits.float()).all()), name
        return rec.calls
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(saved)
        qtip._tables = None
        tmp.cleanup()
        L.gq_reset_env_cache()
        L.gq_set_ap_mode(-1)


# ------------------------------------------------------------------------------------------------ coverage
def _names(calls):
    return [c[0] for c in calls]


def _roles(calls):
    """every role string of a log, descriptor fields included"""
    def walk(v):
        if isinstance(v, str):
            yield v
        elif isinstance(v, dict):
            for e in v.values():
                yield from walk(e)
        elif isinstance(v, list):
            for e in v:
                yield from walk(e)
    return {r for c in calls for r in walk(c[1])}


def _args(calls, name):
    return [c[1] for c in calls if c[0] == name]


def _has(role_prefix):
    return lambda calls: any(r.startswith(role_prefix) for r in _roles(calls))


def _calls(*names):
    return lambda calls: all(n in _names(calls) for n in names)


def _never(*names):
    return lambda calls: not any(n in _names(calls) for n in names)


def _both(*preds):
    return lambda calls: all(p(calls) for p in preds)


def _ks(calls):
    """the split-K part counts of a log's QTIP matvec launches (last scalar of gq_qtip_linear_in)"""
    return [a[11] for a in _args(calls, "gq_qtip_linear_in")]


# (branch, configuration, what its log must show)
COVERAGE = [
    ("AP gate/up pairs on: the pair epilogue (flag 4) through the _ho entry point", "ap4",
     lambda c: any(a[10] == 4 for a in _args(c, "gq_anyprec_gemv_fused_ho")) and "gq_anyprec_gemv_fused" in _names(c)),
    ("AP GQ_NATIVE_PAIRS=0: w2 with silu*mul (flags 1 | 2) through gq_anyprec_gemv_fused", "ap6_no_pairs",
     lambda c: any(a[10] == 3 for a in _args(c, "gq_anyprec_gemv_fused")) and "gq_anyprec_gemv_fused_ho" not in _names(c)),
    ("AP plain wqkv + gq_attn_decode_split", "ap4", _both(_calls("gq_anyprec_gemv_fused", "gq_attn_decode_split"), _never("gq_attn_decode_roped"))),
    ("AP gq_anyprec_gemv_qkv_rope_ho + gq_attn_decode_roped", "ap2_8b_qkv_rope", _calls("gq_anyprec_gemv_qkv_rope_ho", "gq_attn_decode_roped")),
    ("AP GQ_QKV_ATTN=1: one launch", "ap2_8b_qkv_attn", _both(_calls("gq_anyprec_gemv_qkv_rope_attn"), _has("attn_flags+"), _never("gq_attn_decode_roped"))),
    ("AP QK-norm", "ap4_qk_norm", _both(_calls("gq_attn_decode_split_qknorm"), _has("layers.1.attention.q_norm.weight+"))),
    ("AP GQ_SSQ_HANDOVER=1: slots passed to the embedding, the GEMVs and planned per layer", "ap2_8b_handover",
     lambda c: _calls("gq_anyprec_handover_plan")(c) and any(a[5] == "ssq+0" for a in _args(c, "gq_embed_lookup_ho"))
     and any(a[13] == "ssq+0" for a in _args(c, "gq_anyprec_gemv_fused_ho")) and any(a[14] == "ssq+0" for a in _args(c, "gq_anyprec_gemv_fused_ho"))),
    ("AP hand-over off: no plan query, no slots", "ap4", lambda c: _never("gq_anyprec_handover_plan")(c) and not _has("ssq+")(c)),
    ("AP cache > 1024, grouped heads: attn_split > 4 with a workspace", "ap2_8b_long_cache",
     lambda c: all(a[10] > 4 and a[11] == "attn_ws+0" for a in _args(c, "gq_attn_decode_roped")) and _calls("gq_attn_decode_roped")(c)),
    ("AP cache > 1024, GQ_ATTN_GQA=0: attn_split 4", "ap2_8b_long_cache_no_gqa",
     lambda c: all(a[10] == 4 for a in _args(c, "gq_attn_decode_roped")) and _calls("gq_attn_decode_roped")(c)),
    ("AP cache > 1024, plain branch: attn_split 4", "ap4_long_cache",
     lambda c: all(a[12] == 4 and a[13] == "attn_ws+0" for a in _args(c, "gq_attn_decode_split")) and _calls("gq_attn_decode_split")(c)),
    ("AP GQ_ATTN_SPLIT=2", "ap4_attn_split_knob", lambda c: all(a[12] == 2 for a in _args(c, "gq_attn_decode_split")) and _calls("gq_attn_decode_split")(c)),
    ("AP short cache: one split, no workspace", "ap4", lambda c: all(a[12] == 1 and a[13] == "null" for a in _args(c, "gq_attn_decode_split"))),
    ("AP ap_ws present", "ap2_down_workspace", _has("ap_ws+")),
    ("AP 4-bit", "ap4", lambda c: all(a[6] == 4 for a in _args(c, "gq_anyprec_gemv_fused_ho"))),
    ("AP 6-bit", "ap6_no_pairs", lambda c: all(a[6] == 6 for a in _args(c, "gq_anyprec_gemv_fused"))),
    ("QTIP power-of-two widths: 8 launches per layer, q / k / v rebuilt by the attention launch", "qtip_pow2",
     _both(_calls("gq_qtip_linear_in", "gq_qtip_linear_out_seg", "gq_attn_decode_qtip"), _never("gq_qtip_transform", "gq_attn_decode_split"))),
    ("QTIP split K of single linears", "qtip_pow2_4096", lambda c: any(a[11] > 1 for a in _args(c, "gq_qtip_linear_in") if a[7] == 1)),
    ("QTIP split K of the q / k / v group", "qtip_pow2_wide", lambda c: any(a[11] > 1 for a in _args(c, "gq_qtip_linear_in") if a[7] == 3)),
    ("QTIP factor MLP width, GQ_QTIP_MLP_MID on", "qtip_factor_mlp_mid", _both(_calls("gq_qtip_mlp_mid", "gq_qtip_linear_in_rows"), _never("gq_qtip_transform"))),
    ("QTIP factor MLP width, GQ_QTIP_MLP_MID=0", "qtip_factor_no_mlp_mid", _both(_calls("gq_qtip_transform"), _never("gq_qtip_mlp_mid", "gq_qtip_linear_in_rows"))),
    ("QTIP GQ_QTIP_ATTN_FOLD=0", "qtip_no_attn_fold", _both(_calls("gq_attn_decode_split"), _never("gq_attn_decode_qtip"))),
    ("QTIP GQ_QTIP_OUT_SEG=0", "qtip_no_out_seg", _both(_calls("gq_qtip_linear_out"), _never("gq_qtip_linear_out_seg"))),
    ("QTIP GQ_QTIP_KSPLIT=0", "qtip_no_ksplit", lambda c: max(_ks(c)) == 1),
    ("QTIP GQ_QTIP_KSPLIT=0, q / k / v group", "qtip_no_ksplit_wide", lambda c: max(_ks(c)) == 1),
    ("QTIP GQ_QTIP_KSPLIT_GROUP=0", "qtip_no_ksplit_group", lambda c: max(_ks(c)) == 1),
    ("QTIP GQ_QTIP_FOLD=1: a matvec launch that rebuilds its producer's output", "qtip_fold", lambda c: any(a[9] == 1 for a in _args(c, "gq_qtip_linear_in"))),
    ("QTIP GQ_QTIP_ONE_LAUNCH=1", "qtip_one_launch", _both(_calls("gq_qtip_linear"), _never("gq_qtip_linear_out", "gq_qtip_linear_out_seg"))),
    ("QTIP GQ_QTIP_PRE=1", "qtip_pre", _both(_calls("gq_qtip_linear_out_in"), _has("xt[2]+"))),
    ("QTIP cache > 1024: attn_split 4", "qtip_long_cache", lambda c: all(a[12] == 4 and a[13] == "attn_ws+0" for a in _args(c, "gq_attn_decode_qtip"))),
]


def missing_coverage(logs):
    """the branches of COVERAGE a set of logs does not show"""
    return [what for what, name, pred in COVERAGE if not pred(logs[name])]
