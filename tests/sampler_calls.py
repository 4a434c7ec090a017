"""What every decode route asks of the fused sampler's C ABI, as a log that two commits can be compared by (the model of
tests/decode_calls.py, whose `Recorder` does the logging).

For each configuration of `CONFIGS` the recorder goes in for the ctypes library (`_lib._lib`) BEFORE the route's object is built, so the
log holds the constructor's set builds and warm-up draws, the draws made while the graphs are captured and whatever the request sets
up -- every `gq_sample_topk*` and `gq_token_set_build` call in order: the entry point, every scalar as it is, every pointer as a ROLE.
The roles are the sampler's own fields (`counter`, `work_val`, `work_idx`, `ban`, `seq`, `seen`, `suppress`, `lp_ws`, `lp_raw`,
`lp_drawn`) plus `tok`, `pos`, `next_tok`, `logits`, `embed`, `x`, `ssq`, each with its byte offset; `null` for None, `anon` for
anything else (a stream, the id list of a set build).  A route builds its tensors inside the call that is recorded, so pointers are
kept as addresses until the run is over and named then (`sampler_tensors`: the one place that knows where a route keeps them).

tools/record_sampler_calls.py writes the log of a commit to tests/golden/sampler_calls.json (and refuses to when an entry point of
`COVERAGE` is missing from it); tests/test_sampler_calls_golden_gpu.py replays the configurations and compares for equality.
"""
from decode_calls import SMALL, Recorder

FIELDS = ("counter", "work_val", "work_idx", "ban", "seq", "seen", "suppress", "lp_ws", "lp_raw", "lp_drawn")
PROMPT = [3, 17, 5, 60, 2, 9]
EOS = 7


def sampler_tensors(obj):
    """role -> tensor of the sampler state of a route's object (DecodeGraph, _CapturedStep, PipelinedDecoder)"""
    return {f: getattr(obj.sampler, f) for f in FIELDS}


def _step_tensors(obj):
    """role -> tensor of the words a route's step hands to the draw next to the sampler's own"""
    if hasattr(obj, "_tok_out4"):  # (the pipeline: one row of 16 bytes per slot, no token / position feedback)
        return dict(next_tok=obj._tok_out4)
    return dict(tok=obj.tok, pos=obj.pos, next_tok=obj.next_tok if hasattr(obj, "next_tok") else obj.nxt, logits=getattr(obj, "logits", None))


def _model_tensors(m):
    st = m._native_state()
    return dict(logits=st["logits"], x=st["x"], ssq=st["ssq"], embed=m.tok_embeddings.weight)


class _Ptr:
    def __init__(self, p):
        self.p = p


class _LateRecorder(Recorder):
    """`Recorder` with the pointers named after the run"""

    def __init__(self, real):
        super().__init__(real, [])

    def role(self, p):
        return _Ptr(p)

    def log(self, *tensor_dicts):
        """the sampler's calls so far, pointers named by the tensors given; the record starts over"""
        regions = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name)
                   for d in tensor_dicts for name, t in d.items() if t is not None and t.numel()]
        named = Recorder(None, regions)
        calls, self.calls = self.calls, []

        def role(n, i, a):
            # (the id list of a set build is the caller's temporary, freed when the call returns: by the end of the run a tensor made
            # later may sit at its address, so it is never looked up)
            return ("anon" if a.p else "null") if (n, i) == ("gq_token_set_build", 0) else named.role(a.p)
        return [[n, [role(n, i, a) if isinstance(a, _Ptr) else a for i, a in enumerate(args)]]
                for n, args in calls if n.startswith("gq_sample_topk") or n == "gq_token_set_build"]


def _decode_model():
    import torch
    from guidedquant_amd import model as gm
    from guidedquant_amd.generate import load_model
    name = "sampler-calls-ap"
    gm.transformer_configs[name] = dict(dict(model_name="llama-sampler-calls", block_size=2048, n_layer=2, rope_base=500000), **SMALL)
    try:
        m = load_model(name, "cuda:0", "ap", 4, random_init=True)
    finally:
        del gm.transformer_configs[name]
    with torch.device("cuda:0"):
        m.setup_caches(max_batch_size=1, max_seq_length=64)
    return m


def _graph(rec, steps=("step", ), history=None, **kw):
    """a DecodeGraph with the fused sampler, the steps asked for (replays: no calls of their own), and what it asked on the way"""
    import torch
    from guidedquant_amd.generate import DecodeGraph
    m = _decode_model()
    with torch.no_grad():
        g = DecodeGraph(m, "cuda:0", native_sampling=True, temperature=0.8, **dict(dict(top_k=8), **kw))
        g.set_token(5, 3)
        if history is not None:
            g.set_history(history)
        for s in steps:
            getattr(g, s)()
        torch.cuda.synchronize()
    log = rec.log(sampler_tensors(g), _step_tensors(g), _model_tensors(m))
    g.close()
    return log


def _hf_model():
    import torch
    import transformers
    from guidedquant_amd.AnyPrecisionForCausalLM import AnyPrecisionForCausalLM
    cfg = transformers.LlamaConfig(hidden_size=SMALL["dim"], intermediate_size=SMALL["intermediate_size"], num_hidden_layers=2,
                                   num_attention_heads=SMALL["n_head"], num_key_value_heads=SMALL["n_local_heads"], vocab_size=SMALL["vocab_size"],
                                   max_position_embeddings=64, rms_norm_eps=1e-5, tie_word_embeddings=False)
    names = ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"]
    cfg.anyprec = dict(seed_precision=4, parent_precision=4, group_count=1, arch_config=dict(module_names=names, model_name="model", layers_name="layers"))
    return AnyPrecisionForCausalLM.from_config_random(cfg, device=torch.device("cuda:0"), seed=5)


def _generate(rec, capture, **kw):
    """one `generate` request on route 1 (capture=False) or route 2: 5 new tokens, an EOS that min_new_tokens=2 bans at first"""
    import torch
    m = _hf_model()
    ids = torch.tensor([PROMPT], device=m.device)
    route = dict(capture=True, native=False) if capture else dict(native=True)
    out = m.generate(ids, max_new_tokens=5, min_new_tokens=2, eos_token_id=EOS, pad_token_id=0, **route, **kw)
    torch.cuda.synchronize()
    assert out.shape[1] <= len(PROMPT) + 5
    obj = next(v for k, v in m._native_cache.items() if k[0] == ("cap" if capture else "graph"))
    log = rec.log(sampler_tensors(obj), _step_tensors(obj), {} if capture else _model_tensors(m._native_cache[("decoder", 4)]))
    m._drop_native()
    return log


def _pipeline(rec):
    import torch
    from guidedquant_amd.pipeline import PipelinedDecoder
    m = _decode_model()
    dec = PipelinedDecoder(m, 0, 1, range(0, m.config.n_layer), n_seq=1, max_new_tokens=4, temperature=0.8, top_k=8, bos_id=1, native=True)
    with torch.no_grad():
        dec.run(2)
    torch.cuda.synchronize()
    log = rec.log(sampler_tensors(dec), _step_tensors(dec), _model_tensors(m))
    for g in dec.graphs:
        g.reset()
    return log


_REP = dict(do_sample=True, top_k=8, top_p=0.9, temperature=0.7, repetition_penalty=1.3, suppress_tokens=[3, 5])

CONFIGS = {
    "graph_plain": lambda r: _graph(r),
    "graph_top_p": lambda r: _graph(r, top_p=0.9),
    "graph_top_k40": lambda r: _graph(r, top_k=40),
    "graph_fold_seq_two_steps": lambda r: _graph(r, steps=("step", "step_one"), fold_embed=True, seq_capacity=65, steps_per_replay=2),
    "graph_penalty": lambda r: _graph(r, history=PROMPT, repetition_penalty=1.3),
    "graph_suppress": lambda r: _graph(r, suppress_tokens=[3, 5]),
    "graph_logprobs": lambda r: _graph(r, seq_capacity=65, logprobs=True),
    "graph_logprobs_penalty": lambda r: _graph(r, history=PROMPT, seq_capacity=65, logprobs=True, repetition_penalty=1.3),
    "route1_plain": lambda r: _generate(r, False),
    "route1_penalty_suppress": lambda r: _generate(r, False, **_REP),
    "route2_plain": lambda r: _generate(r, True),
    "route2_penalty_suppress": lambda r: _generate(r, True, **_REP),
    "pipeline": _pipeline,
}

# configuration -> the entry points its log must hold, and no other
COVERAGE = {
    "graph_plain": {"gq_sample_topk_p"},
    "graph_top_p": {"gq_sample_topk_p"},
    "graph_top_k40": {"gq_sample_topk_p"},
    "graph_fold_seq_two_steps": {"gq_sample_topk_p"},
    "graph_penalty": {"gq_sample_topk_rep", "gq_token_set_build"},
    "graph_suppress": {"gq_sample_topk_rep", "gq_token_set_build"},
    "graph_logprobs": {"gq_sample_topk_lp"},
    "graph_logprobs_penalty": {"gq_sample_topk_lp", "gq_token_set_build"},
    "route1_plain": {"gq_sample_topk_p"},
    "route1_penalty_suppress": {"gq_sample_topk_rep", "gq_token_set_build"},
    "route2_plain": {"gq_sample_topk_p"},
    "route2_penalty_suppress": {"gq_sample_topk_rep", "gq_token_set_build"},
    "pipeline": {"gq_sample_topk"},
}


def record(name):
    """the sampler calls of configuration `name`"""
    import torch
    from guidedquant_amd import _lib
    from guidedquant_amd.generate import prime_graph_rng_state
    L = _lib.lib()
    prime_graph_rng_state("cuda:0")
    _lib.current_stream_ptr()  # (the one-time self-check of the library runs here, not inside the log)
    torch.manual_seed(0)
    rec = _LateRecorder(L)
    _lib._lib = rec
    try:
        return CONFIGS[name](rec)
    finally:
        _lib._lib = L


def missing_coverage(logs):
    """the configurations whose log does not hold exactly the entry points it is there for"""
    return [name for name, want in COVERAGE.items() if {c[0] for c in logs.get(name, [])} != want]
