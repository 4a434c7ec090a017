"""CPU: the host side of packed scoring -- the packer (guidedquant_amd.native_prompt.pack_plan), the packed mask of the pass
(native_prompt.packed_mask) and of the host model (tests/prefill_packed_model.py) against the per-sequence causal masks placed on the
diagonal, the float64 reference against prefill_attn_model.reference sequence by sequence, and the window of the one-sequence launch a
packed row equals."""
import random

import pytest

torch = pytest.importorskip("torch")

import prefill_attn_model as pam  # noqa: E402
import prefill_packed_model as ppm  # noqa: E402


def _length_sets():
    rnd = random.Random(11)
    sets = [[5], [300], [2, 2, 2], [100, 100, 100, 100], [64, 1, 63, 65, 200, 3], [257, 256, 255, 1, 1]]
    sets += [[rnd.randint(1, 300) for _ in range(n)] for n in (2, 7, 40, 200)]
    return sets


@pytest.mark.parametrize("capacity", [1, 64, 256, 1000])
def test_pack_plan_properties(capacity):
    from guidedquant_amd.native_prompt import pack_plan
    for lens in _length_sets():
        packs = pack_plan(lens, capacity)
        flat = [i for p in packs for i in p]
        assert sorted(flat) == list(range(len(lens)))  # every index exactly once
        assert all(p == sorted(p) for p in packs)  # the input order inside a pack
        assert [p[0] for p in packs] == sorted(p[0] for p in packs)  # and across packs: ordered by their first index
        for p in packs:
            if len(p) > 1:
                assert sum(lens[i] for i in p) <= capacity
            if lens[p[0]] > capacity:
                assert len(p) == 1  # an over-long sequence is alone
        for i, n in enumerate(lens):  # first fit: no earlier pack had room when the sequence was placed
            mine = next(j for j, p in enumerate(packs) if i in p)
            for j in range(mine):
                used = sum(lens[k] for k in packs[j] if k < i)
                assert used + n > capacity or lens[packs[j][0]] > capacity
        assert pack_plan(list(lens), capacity) == packs  # deterministic
        assert pack_plan(tuple(lens), capacity) == packs


def test_pack_plan_examples_and_bad_arguments():
    from guidedquant_amd.native_prompt import pack_plan
    assert pack_plan([], 10) == []
    assert pack_plan([4, 4, 4], 8) == [[0, 1], [2]]
    assert pack_plan([6, 5, 2, 3], 8) == [[0, 2], [1, 3]]  # first fit, not next fit: 2 goes back into the first pack
    assert pack_plan([9, 1, 8], 8) == [[0], [1], [2]]  # nothing joins an over-long sequence
    with pytest.raises(ValueError):
        pack_plan([3], 0)
    with pytest.raises(ValueError):
        pack_plan([3, 0], 8)


@pytest.mark.parametrize("window", [0, 1, 2, 65])
def test_packed_mask_is_the_sequences_masks_on_the_diagonal(window):
    from guidedquant_amd.native_prompt import packed_mask
    for S in (1, 63, 64, 65, 131):
        for name, lens in ppm.layouts(S).items():
            sb = ppm.seg_begin_of(lens)
            assert sb.numel() == S and bool((sb[1:] >= sb[:-1]).all()) and bool((sb <= torch.arange(S)).all())
            want = torch.zeros(S, S, dtype=torch.bool)
            b = 0
            for n in lens:
                want[b:b + n, b:b + n] = pam.attend_mask(n, 0, n, window)
                b += n
            assert torch.equal(ppm.attend_mask_packed(sb, window), want), (S, name)
            assert torch.equal(packed_mask(sb, window or None), want), (S, name)
            # the window of the one-sequence launch: row i of attend_mask(i + 1, 0, i + 1, w_i) is the packed row
            for i, w in enumerate(ppm.row_window(sb, window)):
                one = pam.attend_mask(i + 1, 0, i + 1, 0 if w >= i + 1 else w)[i]
                assert torch.equal(one, want[i, :i + 1]), (S, name, i)


def test_layouts_hold_what_they_promise():
    assert ppm.layouts(1) == {"one": [1]}
    lay = ppm.layouts(131)
    assert lay["cuts"] == [1, 62, 1, 1, 66] and lay["astride"] == [40, 60, 31] and lay["ones"] == [1] * 131
    assert ppm.layouts(64)["cuts"] == [1, 62, 1] and "astride" not in ppm.layouts(64)
    assert ppm.layouts(65)["astride"] == [40, 25]


def test_reference_is_the_one_sequence_reference_per_segment():
    g = torch.Generator().manual_seed(3)
    H, Hkv, hd, S = 4, 2, 64, 70
    q = torch.randn(H, S, hd, generator=g).half()
    K = torch.randn(Hkv, S + 3, hd, generator=g).half()
    V = torch.randn(Hkv, S + 3, hd, generator=g).half()
    pam.poison_rows(K, V, S)
    lens = [10, 1, 40, 19]
    for window in (0, 2, 33):
        got = ppm.reference(q, K, V, ppm.seg_begin_of(lens), 0.125, window)
        assert bool(torch.isfinite(got).all())
        b = 0
        for n in lens:
            want = pam.reference(q[:, b:b + n].contiguous(), K[:, b:b + n].contiguous(), V[:, b:b + n].contiguous(), 0, 0.125, window)
            assert float((got[b:b + n] - want).abs().max()) <= 1e-12
            b += n
