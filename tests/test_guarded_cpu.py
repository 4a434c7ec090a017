"""tests/guarded.py can fail: every kind of damage it is there to detect is reported, on CPU tensors."""
import numpy as np
import pytest
import torch

import guarded
from guarded import GUARD, POISON, Guarded, GuardViolation, Guards


def _buf(n=10):
    return Guarded(np.arange(n, dtype=np.float16), device="cpu", name="x")


def test_layout_and_pattern():
    assert GUARD % 512 == 0 and GUARD >= 4096 and POISON == 0x7E
    b = _buf(5)   # 10 bytes: the payload's end is not aligned to anything, the back guard still starts right behind it
    assert b.nbytes == 10 and b.buf.numel() == 2 * GUARD + 10
    assert b.ptr() == b.buf.data_ptr() + GUARD and b.ptr() % 512 == b.buf.data_ptr() % 512
    assert b.buf.numel() - (GUARD + b.nbytes) >= GUARD
    assert b.view(torch.float16).tolist() == [0, 1, 2, 3, 4]
    assert b.view(torch.float16, (5, 1)).shape == (5, 1)
    assert b.view(torch.float16).data_ptr() == b.ptr()
    assert (b.buf[:GUARD] == POISON).all() and (b.buf[GUARD + 10:] == POISON).all()
    b.check()
    # the meanings the module docstring states
    assert np.isnan(np.array([0x7E7E], dtype=np.uint16).view(np.float16)[0])
    assert 8.3e37 < np.array([0x7E7E7E7E], dtype=np.uint32).view(np.float32)[0] < 8.5e37


def test_clean_buffer_passes_and_payload_writes_are_free():
    b = _buf()
    b.view(torch.float16)[:] = 7
    b.check("x")


@pytest.mark.parametrize("off,side,rel", [
    (lambda b: GUARD + b.nbytes, "back", lambda b: b.nbytes),            # one past the payload
    (lambda b: GUARD - 1, "front", lambda b: -1),                        # one before it
    (lambda b: 0, "front", lambda b: -GUARD),                            # the far end of the front guard
    (lambda b: b.buf.numel() - 1, "back", lambda b: b.nbytes + GUARD - 1),  # the far end of the back guard
])
def test_one_dirty_guard_byte_raises(off, side, rel):
    b = _buf()
    b.buf[off(b)] = 0
    with pytest.raises(GuardViolation) as e:
        b.check("the-buffer")
    msg = str(e.value)
    r = rel(b)
    assert "the-buffer" in msg and side in msg and "1 byte(s)" in msg and f"[{r}, {r}]" in msg


def test_report_names_first_last_and_count():
    b = _buf()
    b.buf[GUARD + b.nbytes + 3] = 1
    b.buf[GUARD + b.nbytes + 40] = 1
    with pytest.raises(GuardViolation, match=r"x: back guard overwritten: 2 byte\(s\), payload offsets \[23, 60\]"):
        b.check()


def test_a_store_of_the_pattern_itself_is_the_only_blind_spot():
    """(documented limit: a stray store of 0x7E bytes cannot be seen; kernels store results, not 0x7E7E)"""
    b = _buf()
    b.buf[GUARD + b.nbytes] = POISON
    b.check()


def test_input_read_one_past_the_end_is_nan():
    b = _buf(10)
    v = b.view(torch.float16)
    over = torch.as_strided(v, (11, ), (1, ))   # inside the allocation: element 10 is the first two guard bytes
    assert not torch.isnan(over[:10]).any() and torch.isnan(over[10])
    before = torch.as_strided(b.buf.view(torch.float16), (1, ), (1, ), GUARD // 2 - 1)
    assert torch.isnan(before[0])
    # fp32 and plane words
    f = Guarded(np.ones(3, np.float32), device="cpu")
    assert float(torch.as_strided(f.view(torch.float32), (4, ), (1, ))[3]) > 8e37
    w = Guarded(np.zeros(3, np.int32), device="cpu")
    assert int(torch.as_strided(w.view(torch.int32), (4, ), (1, ))[3]) == 0x7E7E7E7E


def test_outputs_start_poisoned():
    o = Guarded.empty(6, device="cpu", name="out")
    assert torch.isnan(o.view(torch.float16)).all()
    assert (o.numpy(np.uint8) == POISON).all()


def test_guards_collection_reports_the_buffer_name():
    g = Guards(device="cpu")
    g.inp("x", np.zeros(4, np.float16))
    o = g.out("out", 8)
    assert g.inp("residual", None) is None and guarded.ptr(None) is None
    g.check()
    o.buf[GUARD + 8] = 0
    with pytest.raises(GuardViolation, match=r"^out: back guard overwritten: 1 byte\(s\), payload offsets \[8, 8\]"):
        g.check()


def test_bad_guard_size_is_refused():
    with pytest.raises(AssertionError):
        Guarded.empty(4, device="cpu", guard=1000)
    with pytest.raises(AssertionError):
        Guarded.empty(4, device="cpu", guard=512)
