"""CPU: the two host decisions of the prompt pass (guidedquant_amd/native_prompt.py) as truth tables, written out from the expressions
`Transformer._prompt_pass` and `Transformer.score_native` held before the pass moved:
    fp16 cache: hip = mode != "0" and (mode == "1" or pieces > 1) and supported            -> "hip" | "sdpa"
    fp8 cache:  hip = mode != "0" and supported                                            -> "hip-kv8" | "sdpa-kv8"
    head:       kernel = mode == "1" or (mode == "auto" and served and SCORE_HEAD_AUTO == "1")"""
import pytest

from guidedquant_amd.native_prompt import attention_plan, score_head_choice

# (mode, pieces, kv8, supported) -> plan: 3 modes x {1, 2 pieces} x kv8 x supported
PLAN = {
    ("auto", 1, False, False): "sdpa", ("auto", 1, False, True): "sdpa",
    ("auto", 2, False, False): "sdpa", ("auto", 2, False, True): "hip",
    ("auto", 1, True, False): "sdpa-kv8", ("auto", 1, True, True): "hip-kv8",
    ("auto", 2, True, False): "sdpa-kv8", ("auto", 2, True, True): "hip-kv8",
    ("0", 1, False, False): "sdpa", ("0", 1, False, True): "sdpa",
    ("0", 2, False, False): "sdpa", ("0", 2, False, True): "sdpa",
    ("0", 1, True, False): "sdpa-kv8", ("0", 1, True, True): "sdpa-kv8",
    ("0", 2, True, False): "sdpa-kv8", ("0", 2, True, True): "sdpa-kv8",
    ("1", 1, False, False): "sdpa", ("1", 1, False, True): "hip",
    ("1", 2, False, False): "sdpa", ("1", 2, False, True): "hip",
    ("1", 1, True, False): "sdpa-kv8", ("1", 1, True, True): "hip-kv8",
    ("1", 2, True, False): "sdpa-kv8", ("1", 2, True, True): "hip-kv8",
}

# (mode, served, SCORE_HEAD_AUTO) -> the kernel
HEAD = {
    ("auto", False, "0"): False, ("auto", False, "1"): False, ("auto", True, "0"): False, ("auto", True, "1"): True,
    ("0", False, "0"): False, ("0", False, "1"): False, ("0", True, "0"): False, ("0", True, "1"): False,
    ("1", False, "0"): True, ("1", False, "1"): True, ("1", True, "0"): True, ("1", True, "1"): True,
}


def test_attention_plan_truth_table():
    assert len(PLAN) == 3 * 2 * 2 * 2
    for args, want in PLAN.items():
        assert attention_plan(*args) == want, args
    for n in (3, 5):  # (more pieces than two: a chunked pass like two)
        for (mode, _, kv8, sup), want in ((k, v) for k, v in PLAN.items() if k[1] == 2):
            assert attention_plan(mode, n, kv8, sup) == want


@pytest.mark.parametrize("kv8", [False, True])
def test_a_bad_attention_mode_is_named(kv8):
    with pytest.raises(ValueError, match="GQ_PREFILL_ATTN='maybe': auto, 0 or 1"):
        attention_plan("maybe", 2, kv8, True)


def test_score_head_choice_truth_table():
    assert len(HEAD) == 3 * 2 * 2
    for args, want in HEAD.items():
        assert score_head_choice(*args) is want, args
    with pytest.raises(ValueError, match="GQ_SCORE_HEAD='2': auto, 0 or 1"):
        score_head_choice("2", True, "1")


def test_the_moved_names_stay_importable_from_the_model_module():
    from guidedquant_amd import model, native_prompt
    assert model.prefill_chunks is native_prompt.prefill_chunks and model._sdpa_gqa is native_prompt._sdpa_gqa
    assert model.prefill_chunks(17, 16) == [(0, 16), (16, 1)]
    for name in ("mask_rows", "window_mask", "MASK_TABLE_MAX", "fp8_quantize", "kv_cache_dtype_name"):
        assert hasattr(model, name), name
    assert model.Transformer.SCORE_HEAD_ROWS == 512 and model.Transformer.SCORE_HEAD_AUTO in ("0", "1")
