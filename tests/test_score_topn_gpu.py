"""GPU: `score(..., top_logprobs=n)` on the fused route -- the HIP prompt pass with gq_head_nll_topn on every piece -- on the tiny models of
test_score_native_gpu.py (V = 1000 / 777 / 500: no multiple of the kernel's tile; S = 131: two row tiles).
  * the keyword changes nothing else: logprobs / greedy / nll of score(ids, top_logprobs=5) are score(ids)'s bit for bit; entry 0 of a list
    is the target wherever `greedy` says so; the target's entry is `logprobs` bit for bit wherever it is listed;
  * a chunked pass (GQ_PREFILL_CHUNK=48: pieces of 48, 48, 35 rows) lists the ids of the one-piece pass;
  * the torch head (GQ_SCORE_HEAD=0) lists the same ids at every position whose logit differs from both neighbours in the reference's
    sorted row (equal fp16 neighbours may come in either order between two heads that round on their own); at most 5 % of the positions
    may be left out, counted on the host from the reference logits alone.  Log-probabilities: test_score_native_gpu.py's rule between two
    heads, 2 ulp16(max |logit| of the row).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_score_native_gpu as tsn  # noqa: E402

N = 5


def test_the_keyword_changes_nothing_else(monkeypatch):
    monkeypatch.delenv("GQ_PREFILL_ATTN", raising=False)
    monkeypatch.setenv("GQ_SCORE_HEAD", "1")
    m = tsn._hf_tiny()
    d = m.device
    ids = torch.randint(0, 500, (150, ), device=d, generator=torch.Generator(device=d).manual_seed(3))
    plain, r = m.score(ids), m.score(ids, top_logprobs=N)
    assert m._native_cache[("decoder", 2)].last_prefill_plan["head"] == "hip-nll-topn"
    assert sorted(plain) == ["greedy", "logprobs", "nll"] and sorted(r) == ["greedy", "logprobs", "nll", "top_logprobs", "top_logprobs_ids"]
    assert torch.equal(r["logprobs"], plain["logprobs"]) and torch.equal(r["greedy"], plain["greedy"]) and r["nll"] == plain["nll"]
    tid, tlp = r["top_logprobs_ids"], r["top_logprobs"]
    assert tid.shape == (149, N) and tid.dtype == torch.int64 and tlp.shape == (149, N) and tlp.dtype == torch.float32
    assert bool((tid >= 0).all()) and bool((tid < 500).all()) and bool((tlp[:, :-1] >= tlp[:, 1:]).all())
    # random targets are rarely listed: the last token replaced by entry 0, then by entry 2, of its own row's list (no row sees it as context)
    for k in (0, 2):
        ids_k = ids.clone()
        ids_k[-1] = tid[-1, k]
        rk = m.score(ids_k, top_logprobs=N)
        assert torch.equal(rk["top_logprobs_ids"], tid) and torch.equal(rk["top_logprobs"], tlp)
        assert bool(rk["greedy"][-1]) == (k == 0) and torch.equal(tid[:, 0] == ids_k[1:], rk["greedy"])
        hit = tid == ids_k[1:, None]
        assert bool(hit[-1, k]) and torch.equal(tlp[hit], rk["logprobs"][:, None].expand_as(tlp)[hit])
    with pytest.raises(ValueError, match="top_logprobs: "):
        m.score(ids, top_logprobs=21)


def _lists(m, idx, monkeypatch, head, chunk=None):
    monkeypatch.setenv("GQ_SCORE_HEAD", head)
    if chunk is not None:
        monkeypatch.setenv("GQ_PREFILL_CHUNK", str(chunk))
    with torch.no_grad():
        lp, greedy, tid, tlp = m.score_native(idx, top_logprobs=N)
    monkeypatch.delenv("GQ_PREFILL_CHUNK", raising=False)
    assert tid.shape == (tsn.S - 1, N) and tid.dtype == torch.int64 and tlp.dtype == torch.float32
    return tid.cpu().numpy(), tlp.double().cpu().numpy()


@pytest.mark.parametrize("kind", list(tsn._BUILD))
def test_chunked_pass_and_torch_head_list_the_same_tokens(kind, monkeypatch):
    m, idx, want, tol, clear, greedy = tsn._model(kind)
    monkeypatch.setenv("GQ_PREFILL_ATTN", "1")  # (both passes through the attention kernel: they differ in the chunking alone)
    one, one_lp = _lists(m, idx, monkeypatch, "1")
    assert m.last_prefill_plan["head"] == "hip-nll-topn" and len(m.last_prefill_plan["chunks"]) == 1
    got, _ = _lists(m, idx, monkeypatch, "1", chunk=48)
    assert m.last_prefill_plan["chunks"] == [(0, 48), (48, 48), (96, 35)]
    assert np.array_equal(got, one)
    # the reference's own sorted rows say which positions two heads must agree on
    with torch.no_grad():
        logits = m.prefill_native(idx.view(1, -1), torch.arange(tsn.S, dtype=torch.int32, device=idx.device), start=0, last_only=False)[0, :tsn.S - 1]
    top = -np.sort(-logits.double().cpu().numpy(), axis=1)[:, :N + 1]
    differs = top[:, :-1] != top[:, 1:]  # [rows, N]: position j against j + 1
    firm = differs & np.concatenate([np.ones((top.shape[0], 1), dtype=bool), differs[:, :-1]], axis=1)
    print("%s: %.2f %% of the positions have an fp16-equal neighbour" % (kind, 100.0 * (1.0 - firm.mean())))
    assert 1.0 - firm.mean() <= 0.05
    ref, ref_lp = _lists(m, idx, monkeypatch, "0")
    assert m.last_prefill_plan["head"] == "torch"
    assert np.array_equal(ref[firm], one[firm])
    d = np.abs(ref_lp - one_lp) / tol[:, None]
    print("%s: worst |dlogprob| / (2 ulp16) between the heads' lists %.3f" % (kind, d[firm].max()))
    assert (d[firm] <= 1.0).all()
