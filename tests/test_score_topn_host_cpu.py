"""No GPU: `score(..., top_logprobs=n)` on the module tree (the route a CPU model takes) and the torch definition of a row's list
(native_prompt.top_rows): the keyword's keys, shapes and dtypes, the stable tie order on hand-made logits, the NaN / fill rule, the
named error, and the unchanged dict without the keyword."""
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from test_score_host_cpu import VOCAB, stream, wrapper  # noqa: E402,F401  (the tiny CPU model and its token stream)


def test_keyword_adds_two_lists_and_changes_nothing_else(wrapper, stream):
    ids = stream[:17]
    plain, r = wrapper.score(ids), wrapper.score(ids, top_logprobs=5)
    assert sorted(plain) == ["greedy", "logprobs", "nll"]
    assert sorted(r) == ["greedy", "logprobs", "nll", "top_logprobs", "top_logprobs_ids"]
    assert torch.equal(r["logprobs"], plain["logprobs"]) and torch.equal(r["greedy"], plain["greedy"]) and r["nll"] == plain["nll"]
    tid, tlp = r["top_logprobs_ids"], r["top_logprobs"]
    assert tid.shape == (16, 5) and tid.dtype == torch.int64 and tlp.shape == (16, 5) and tlp.dtype == torch.float32
    with torch.no_grad():
        ls = torch.log_softmax(wrapper.model(input_ids=ids.view(1, -1)).logits[0, :-1].float(), dim=-1)
    assert torch.equal(tlp, ls.gather(1, tid)) and bool((tlp[:, :-1] >= tlp[:, 1:]).all())
    assert torch.equal(tid[:, 0] == ids[1:], r["greedy"])
    hit = tid == ids[1:, None]
    assert torch.equal(tlp[hit], r["logprobs"][:, None].expand_as(tlp)[hit])  # (bit for bit: the same entry of the same log_softmax)
    assert wrapper.score(ids, top_logprobs=20)["top_logprobs_ids"].shape == (16, 20)


def test_equal_logits_come_by_ascending_id_and_a_nan_is_never_listed():
    from guidedquant_amd.native_prompt import top_rows
    nan, inf = float("nan"), float("inf")
    logits = torch.tensor([[1.0, 3.0, 1.0, 3.0, 0.0, 3.0],
                           [0.0, -0.0, 2.0, 2.0, -inf, nan],
                           [nan, -inf, nan, 5.0, nan, nan]], dtype=torch.float16)
    ls = torch.log_softmax(logits.float(), dim=-1)
    ids, lps = top_rows(logits, ls, 4)
    assert ids.tolist() == [[1, 3, 5, 0], [2, 3, 0, 1], [3, 1, -1, -1]]
    assert ids.dtype == torch.int64 and lps.dtype == torch.float32
    assert torch.equal(lps[0], ls[0, ids[0]]) and bool(torch.isnan(lps[1]).all())  # (a NaN in the row: its lse is NaN)
    assert lps[2, 2:].tolist() == [-inf, -inf]
    ids, lps = top_rows(logits[:1, :3], ls[:1, :3], 5)  # a vocabulary smaller than n
    assert ids.tolist() == [[1, 0, 2, -1, -1]] and lps[0, 3:].tolist() == [-inf, -inf]


@pytest.mark.parametrize("n", [0, 21, True, 2.0])
def test_a_bad_count_is_named(wrapper, stream, n):
    with pytest.raises(ValueError, match="top_logprobs: "):
        wrapper.score(stream[:8], top_logprobs=n)
