"""GPU: gq_attn_decode_split_kv8 (csrc/attn_kv8.hip) -- the fp8 cache's decode attention that rotates, quantises, writes the cache row and
attends in ONE launch -- and the route behind GQ_KV8_FOLD=1 (native_step.StepState.attend_kv8).

  chain        the entry leaves, bit for bit, the `out` vector and the cache bytes that gq_rope_cache_rows_kv8 (S = 1) followed by
               gq_attn_decode_roped_kv8 leave for the same n_split and window (the contract of include/gq_hip.h), on guard-banded buffers:
               the row *pos written, every other cache byte as it was.  Positions (n_split): 0 (1), 1 (4), the last row of a pass (1), the
               first row of the next (4), 2 PASS (4: the first context that is split), 2 PASS + 1 (3: the current token in the last
               split; 4: a split that starts behind *pos).
  host model   against float64 over the dequantised cache the launch left (kv8_model.dequant), the criterion and the constant
               tests/test_kv8_attn_gpu.py holds gq_attn_decode_roped_kv8 to; the written row against kv8_model.quantize of the host's rotation.
  model        a prompt and 12 decode steps with GQ_KV8_FOLD=1 against GQ_KV8_FOLD=0: logits and cache bytes bit for bit, one launch per
               layer less, the same tokens from a DecodeGraph with ten steps per replay; the knob unset launches what 0 launches."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import attn_probes as ap  # noqa: E402
import kv8_model as k8  # noqa: E402
from guarded import Guards, ptr  # noqa: E402

EPS = 1e-6


def _L():
    from guidedquant_amd import _lib
    return _lib


def _pass(hd):
    return ap.geometry(hd, 0, 1).PASS


def _cases(hd):
    P = _pass(hd)
    return [(0, 1), (1, 4), (P - 1, 1), (P, 4), (2 * P, 4), (2 * P + 1, 3), (2 * P + 1, 4)]


_pool = {}


def _inputs(H, Hkv, hd):
    """everything a launch reads but the position and the scales (CPU), generated once per head geometry"""
    key = (H, Hkv, hd)
    if key not in _pool:
        g = torch.Generator().manual_seed(11 + H + 3 * Hkv + hd)
        n = 2 * _pass(hd) + 8
        ang = torch.rand(n, hd // 2, generator=g) * 6.28
        _pool[key] = dict(
            max_seq=n, qkv=torch.randn((H + 2 * Hkv) * hd, generator=g).half(), cos=torch.cat([ang.cos()] * 2, 1).half(), sin=torch.cat([ang.sin()] * 2, 1).half(),
            K=k8.random_codes((Hkv, n, hd), g), V=k8.random_codes((Hkv, n, hd), g), qw=(1 + 0.1 * torch.randn(hd, generator=g)).half(),
            kw=(1 + 0.1 * torch.randn(hd, generator=g)).half(), bias=(0.5 * torch.randn((H + 2 * Hkv) * hd, generator=g)).half())
    return _pool[key]


def _launch(fold, inp, H, Hkv, hd, form, window, ks, vs, pos, ns, qkv=None):
    """one launch of the entry (fold) or of the chain on guarded buffers: (rc, out bits [H, hd], K bytes, V bytes); rows behind *pos (and
    below the window) hold what an earlier sequence left, NaN and 448 codes"""
    _lib = _L()
    L, sp, n = _lib.lib(), _lib.current_stream_ptr(), inp["max_seq"]
    lo = pos + 1 - window if window and pos + 1 > window else 0
    K, V = inp["K"].clone(), inp["V"].clone()
    for c in (K, V):
        c[:, :lo] = k8.stale_rows(lo, hd)
        c[:, min(pos, n):] = k8.stale_rows(n - min(pos, n), hd)
    g = Guards()
    b = {k: g.inp(k, v) for k, v in dict(qkv=inp["qkv"] if qkv is None else qkv, pos=torch.tensor([pos], dtype=torch.int32), cos=inp["cos"], sin=inp["sin"], K=K, V=V,
                                         k_inv=1.0 / ks, v_inv=1.0 / vs, ks=ks, vs=vs, qw=inp["qw"] if form in ("qknorm", "both") else None,
                                         kw=inp["kw"] if form in ("qknorm", "both") else None, bias=inp["bias"] if form in ("bias", "both") else None).items()}
    out, ws = g.out("out", H * hd * 2), g.out("ws", H * ns * (hd + 2) * 4) if ns > 1 else None
    head = (b["qkv"].ptr(), b["pos"].ptr(), b["cos"].ptr(), b["sin"].ptr())
    tail = (ptr(b["qw"]), ptr(b["kw"]), EPS, ptr(b["bias"]))
    if fold:
        rc = L.gq_attn_decode_split_kv8(*head, b["K"].ptr(), b["V"].ptr(), b["k_inv"].ptr(), b["v_inv"].ptr(), b["ks"].ptr(), b["vs"].ptr(), out.ptr(), H, Hkv, hd, n,
                                        ap.default_scale(hd), ns, ptr(ws), *tail, window, sp)
    else:
        q = g.out("q", H * hd * 2)
        rc = L.gq_rope_cache_rows_kv8(*head, q.ptr(), b["K"].ptr(), b["V"].ptr(), b["k_inv"].ptr(), b["v_inv"].ptr(), 1, H, Hkv, hd, n, *tail, sp)
        rc = rc or L.gq_attn_decode_roped_kv8(q.ptr(), b["pos"].ptr(), b["K"].ptr(), b["V"].ptr(), b["ks"].ptr(), b["vs"].ptr(), out.ptr(), H, Hkv, hd, n,
                                              ap.default_scale(hd), ns, ptr(ws), window, sp)
    g.check()
    return rc, out.view(torch.int16, (H, hd)).cpu(), b["K"].view(torch.uint8, K.shape).cpu(), b["V"].view(torch.uint8, V.shape).cpu(), (K, V)


def _same_as_chain(inp, H, Hkv, hd, form, window, ks, vs, pos, ns, qkv=None):
    _lib = _L()
    got, want = (_launch(f, inp, H, Hkv, hd, form, window, ks, vs, pos, ns, qkv) for f in (True, False))
    what = (form, window, float(ks[0]), pos, ns)
    _lib.check(got[0], "gq_attn_decode_split_kv8")
    _lib.check(want[0], "the chain")
    assert torch.equal(got[1], want[1]), ("out", what, int((got[1] != want[1]).sum()))
    for i, name in ((2, "K"), (3, "V")):
        before = got[4][i - 2]
        assert torch.equal(got[i], want[i]), (name, what, int((got[i] != want[i]).sum()))
        if pos < inp["max_seq"]:
            keep = torch.ones(inp["max_seq"], dtype=torch.bool)
            keep[pos] = False
            assert torch.equal(got[i][:, keep], before[:, keep]), (name + ": a byte outside row *pos changed", what)
            assert not torch.equal(got[i][:, pos], before[:, pos]), (name + ": row *pos was not written", what)
        else:
            assert torch.equal(got[i], before), (name + ": written past the cache", what)
    return got


@pytest.mark.parametrize("window", [0, 5])
@pytest.mark.parametrize("form", ["plain", "qknorm", "bias"])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("hd", [64, 128])
def test_entry_equals_the_two_launch_chain_bit_for_bit(hd, H, Hkv, form, window):
    inp = _inputs(H, Hkv, hd)
    for s in (1.0, 2.0**-3, 0.37):
        ks, vs = torch.full((Hkv,), s), torch.full((Hkv,), s)
        for pos, ns in _cases(hd):
            qkv = inp["qkv"].roll(int(37 * pos + 1000 * s))  # (other numbers in every launch: a rounding that differs once in 10^4 shows)
            got = _same_as_chain(inp, H, Hkv, hd, form, window, ks, vs, pos, ns, qkv)
            assert not bool((got[1] == 0x7E7E).any()), "an output element was not written"


@pytest.mark.parametrize("hd", [64, 128])
def test_nonfinite_current_token_and_the_end_of_the_cache(hd):
    H, Hkv = 8, 2
    inp = _inputs(H, Hkv, hd)
    ks, vs = torch.full((Hkv,), 0.37), torch.full((Hkv,), 0.37)
    for where in (H * hd, (H + Hkv) * hd):  # k, then v, of KV group 0: a NaN, +Inf and -Inf, in both halves of the head
        qkv = inp["qkv"].clone()
        qkv[where + 3], qkv[where + hd // 2 + 1], qkv[where + hd - 2] = float("nan"), float("inf"), float("-inf")
        _same_as_chain(inp, H, Hkv, hd, "plain", 0, ks, vs, _pass(hd), 4, qkv)
    got = _same_as_chain(inp, H, Hkv, hd, "plain", 0, ks, vs, inp["max_seq"], 4)  # *pos = max_seq: NaN output, caches untouched
    assert bool((got[1] == 0x7E00).all())


def test_norm_weights_with_a_bias_and_other_head_dims_are_declined():
    _lib = _L()
    one = torch.ones(2)
    assert _launch(True, _inputs(8, 2, 64), 8, 2, 64, "both", 0, one, one, 3, 1)[0] == _lib.GQ_EINVAL
    inp = _inputs(8, 2, 64)
    inp = dict(inp, max_seq=16, K=inp["K"][:, :16, :32].contiguous(), V=inp["V"][:, :16, :32].contiguous())
    rc, out, K, V, before = _launch(True, inp, 8, 2, 32, "plain", 0, one, one, 3, 1)
    assert rc == _lib.GQ_ENOTSUP and bool((out == 0x7E7E).all()) and torch.equal(K, before[0]) and torch.equal(V, before[1])


@pytest.mark.parametrize("H,Hkv,hd", [(8, 2, 64), (4, 4, 128)])
def test_against_the_float64_host_model(H, Hkv, hd):
    inp = _inputs(H, Hkv, hd)
    ks, vs = k8.scale_sets(Hkv)["free"]
    pos, ns = 2 * _pass(hd) + 1, 3
    rc, out, K, V, _ = _launch(True, inp, H, Hkv, hd, "plain", 0, ks, vs, pos, ns)
    _L().check(rc, "gq_attn_decode_split_kv8")
    # the host's rotation, three fp16 operations (apply_rotary_pos_emb), and the write rule on its k and v
    x = inp["qkv"].view(H + 2 * Hkv, hd)
    rot = x * inp["cos"][pos] + torch.cat([-x[:, hd // 2:], x[:, :hd // 2]], 1) * inp["sin"][pos]
    assert torch.equal(K[:, pos], k8.quantize(rot[H:H + Hkv], (1.0 / ks)[:, None])) and torch.equal(V[:, pos], k8.quantize(x[H + Hkv:], (1.0 / vs)[:, None]))
    ref, _, A = ap.reference(rot[:H], k8.dequant(K, ks, torch.float64), k8.dequant(V, vs, torch.float64), pos, ap.default_scale(hd))
    o = out.view(torch.float16).double()
    assert torch.isfinite(o).all()
    excess = (o - ref).abs() - 2.0**-10 * ref.abs()  # (err - 2^-10 |ref|) / A <= c, multiplied out (tests/test_kv8_attn_gpu.py)
    print("H%d/%d hd%d: worst profile ratio %.3e (c = %.3e)" % (H, Hkv, hd, float((excess / A)[A > 0].max()), ap.PROFILE_C))
    assert bool((excess <= ap.PROFILE_C * A).all()), float((excess - ap.PROFILE_C * A).max())


# ------------------------------------------------------------------------------------------------------------------ through the model
S, STEPS, CACHE = 17, 12, 256


def _decode(m, fold, monkeypatch, idx):
    """prompt + STEPS eager steps + one replay of a ten-step DecodeGraph under GQ_KV8_FOLD = fold (None: unset):
    (logits per step, cache bytes behind the eager steps, entry points of one step, the graph's tokens)"""
    from decode_calls import Recorder, regions_of
    from guidedquant_amd.generate import DecodeGraph
    _lib, d = _L(), idx.device
    monkeypatch.delenv("GQ_KV8_FOLD", raising=False) if fold is None else monkeypatch.setenv("GQ_KV8_FOLD", fold)
    _lib.lib().gq_reset_env_cache()
    graph = DecodeGraph(m, d, native_sampling=True, temperature=0.0, top_k=32, seq_capacity=CACHE, steps_per_replay=10)
    try:
        for b in m.layers:
            b.attention.kv_cache.k_cache.view(torch.uint8).zero_()
            b.attention.kv_cache.v_cache.view(torch.uint8).zero_()
        pos = torch.arange(S + STEPS, dtype=torch.int32, device=d)
        logits, names = [], None
        with torch.no_grad():
            m.prefill_native(idx[:, :S], pos[:S], start=0)
            for t in range(S, S + STEPS):
                if t == S:
                    real = _lib.lib()
                    rec = Recorder(real, regions_of(m))
                    _lib._lib = rec
                try:
                    logits.append(m.decode_native(idx[0, t:t + 1], pos[t:t + 1]).view(-1).clone())
                finally:
                    if t == S:
                        _lib._lib, names = real, [c[0] for c in rec.calls]
        caches = [c.view(torch.uint8).clone() for b in m.layers for c in (b.attention.kv_cache.k_cache, b.attention.kv_cache.v_cache)]
        graph.set_token(logits[-1].float().argmax().to(torch.int32), S + STEPS)
        graph.step()
        torch.cuda.synchronize()
        return logits, caches, names, graph.seq[S + STEPS + 1:S + STEPS + 11].clone()
    finally:
        graph.close()


@pytest.mark.parametrize("kind", ["llama-2bit", "window8", "qwen2", "qwen3"])
def test_fold_knob_through_the_model(kind, monkeypatch):
    import test_kv8_model_gpu as tm  # (its tiny models: Llama, Mistral with a window, Qwen2 with a bias, Qwen3 with the QK-norm)
    m = tm._BUILD[kind]()
    m.setup_caches(1, CACHE, kv_cache_dtype="fp8")
    i = torch.arange(len(m.layers) * m.config.n_local_heads, dtype=torch.float32).view(len(m.layers), -1)
    m.set_kv_scales(0.37 + 0.11 * i, 2.9 - 0.3 * i)
    d = tm._dev()
    idx = torch.randint(0, m.config.vocab_size, (1, S + STEPS), dtype=torch.int32, device=d, generator=torch.Generator(device=d).manual_seed(5))
    two, one, unset = (_decode(m, f, monkeypatch, idx) for f in ("0", "1", None))
    chain = ["gq_rope_cache_rows_kv8", "gq_attn_decode_roped_kv8"]
    assert unset[2] == two[2] and all(two[2].count(n) == len(m.layers) for n in chain) and "gq_attn_decode_split_kv8" not in two[2]
    assert [n for n in two[2] if n not in chain] == [n for n in one[2] if n != "gq_attn_decode_split_kv8"]
    assert one[2].count("gq_attn_decode_split_kv8") == len(m.layers) and len(one[2]) == len(two[2]) - len(m.layers)
    for t, (a, b) in enumerate(zip(one[0], two[0])):
        assert torch.isfinite(a.float()).all() and torch.equal(a.view(torch.int16), b.view(torch.int16)), (kind, "logits of step", t)
    assert all(torch.equal(a, b) for a, b in zip(one[1], two[1])), (kind, "cache bytes")
    assert torch.equal(one[3], two[3]) and torch.equal(unset[3], two[3]), (kind, "tokens of the graph", one[3].tolist(), two[3].tolist())
